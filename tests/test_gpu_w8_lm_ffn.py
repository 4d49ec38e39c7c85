"""The one-launch LM MLP kernels on FP8 weights (lm_ffn.hip: the W8 forms of
k_lm_ffn at 1..2 rows and k_lm_ffn16 at 3..16 rows).

The W8 forms keep the bf16 forms' tiles, k-block ranges, MFMA order, LDS sums
and epilogues and convert a fragment to code * 2^e[row] -- exactly the bf16
value -- where the bf16 form reads it.  So an FP8 engine's block must equal,
bit for bit, the bf16 kernel of an engine built from fake_quantize_state_dict.
Against the FP8 GEMV pair (another summation order) and the oracle the bound is
test_gpu_lm.py's for one launch against the pair: rel L2 < 2e-2, cosine > 0.999.

All engines are the smallest these kernels accept (H 1536, I 8960, 2 layers so
the per-layer weight table is exercised), built one after another: a one-launch
kernel runs only while its context is the device's only registered one.
"""
import ctypes
import gc

import pytest
import torch

from gpu_util import cos, rel_err
from oracle import lm as olm
from sync_counters import assert_counters_consistent
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.synthetic import tokenizer_ids
from vibevoice_amd.weights import (W8_CODES, W8_EXPS, dequantize_rows, fake_quantize_state_dict, mfma_pack,
                                   mfma_unpack8, synthetic_state_dict)

pytestmark = pytest.mark.gpu
dev = "cuda"
I32 = dict(dtype=torch.int32, device=dev)
TK = tokenizer_ids()
D, E, S, X = TK.speech_diffusion_id, TK.speech_end_id, TK.speech_start_id, TK.eos_token_id
VALID = [151643, 151652, 151653, 151654]
FP8 = "fp8_e4m3"
H, I = 1536, 8960
LMP = "model.language_model."


@pytest.fixture(autouse=True)
def _switches():
    gc.collect()
    yield
    _lib.lib().vv_lm_ffn(1)
    _lib.lib().vv_lm_ffn_w8(3)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def _cfg():
    return tiny_config(hidden=H, layers=2, heads=12, kv_heads=2, inter=I)


def _sd(cfg, seed):
    return synthetic_state_dict(cfg, seed=seed, device="cpu", mode="test", with_acoustic_encoder=False)


def _engine(cfg, sd, weight_dtype, max_batch, max_ctx=128):
    return Engine(cfg, sd, dev, max_batch=max_batch, max_ctx=max_ctx, valid_ids=VALID, weight_dtype=weight_dtype)


def _oracle_sd(sd):
    return {k[len(LMP):]: v for k, v in sd.items() if k.startswith(LMP)}


# ------------------------------------------------------------------ 1. which path runs
def test_active():
    cfg = _cfg()
    sd = _sd(cfg, 41)
    L = _lib.lib()
    q = _engine(cfg, sd, FP8, max_batch=8)
    rows = (1, 2, 3, 16, 17)
    act = lambda e: [L.vv_lm_ffn_active(e.h, r) for r in rows]   # noqa: E731
    assert q.weights_quantized()
    assert act(q) == [1, 1, 1, 1, 0]
    assert all(L.vv_lm_attn_active(q.h, r, 64) == 0 for r in rows)
    L.vv_lm_ffn(0)
    assert act(q) == [0, 0, 0, 0, 0]
    L.vv_lm_ffn(1)
    assert L.vv_lm_ffn_w8(1) == 0
    assert act(q) == [1, 1, 0, 0, 0]
    assert L.vv_lm_ffn_w8(2) == 0
    assert act(q) == [0, 0, 1, 1, 0]
    assert L.vv_lm_ffn_w8(0) == 0
    assert act(q) == [0, 0, 0, 0, 0]
    q.close()
    gc.collect()
    b = _engine(cfg, sd, None, max_batch=8)          # a bf16 engine does not read the W8 switch
    assert act(b) == [1, 1, 1, 1, 0]
    L.vv_lm_ffn_w8(3)
    assert act(b) == [1, 1, 1, 1, 0]
    b.close()


# ------------------------------------------------------------------ 2. bit identity
ROWS = (1, 2, 3, 6, 16)


def _spread_exponents(cfg, sd):
    """Row n of every layer's packed gate|up matrix (tiles of 8 gate + 8 up rows)
    and of its down matrix times 2^((n mod 13) - 6): the rows of one tile get
    widely different exponents, and since a power of two commutes with the
    quantiser the FP8 and the fake-quantised engines still hold equal values.
    One gate|up row pair and one down row are zero (exponent 0)."""
    def scaled(w, n):
        return torch.ldexp(w.float(), ((n % 13) - 6)[:, None].to(torch.int32)).to(w.dtype)
    r = torch.arange(I)
    for l in range(cfg.decoder_config.num_hidden_layers):
        p = f"{LMP}layers.{l}.mlp."
        g, u, d = (sd[p + n + ".weight"] for n in ("gate_proj", "up_proj", "down_proj"))
        g, u = scaled(g, 16 * (r // 8) + r % 8), scaled(u, 16 * (r // 8) + 8 + r % 8)
        d = scaled(d, torch.arange(H))
        g[19 + 8 * l] = 0
        u[19 + 8 * l] = 0
        d[21 + 16 * l] = 0
        sd[p + "gate_proj.weight"], sd[p + "up_proj.weight"], sd[p + "down_proj.weight"] = g, u, d
    return sd


def _replay(eng, x):
    """Both layers' MLP blocks on a fresh copy of the rows x (in place on the copy)."""
    h = x.clone()
    act = torch.empty(x.shape[0], I, device=dev, dtype=torch.bfloat16)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().vv_lm_mlp_replay(eng.h, x.shape[0], P(h), P(act), 1, st), "lm_mlp_replay")
    torch.cuda.synchronize()
    return h


@pytest.fixture(scope="module")
def blocks():
    """{R: rows}, the FP8 engine's outputs (one launch twice, then the GEMV pair)
    and the bf16 engine's on the fake-quantised weights; computed once."""
    gc.collect()
    L = _lib.lib()
    cfg = _cfg()
    sd = _spread_exponents(cfg, _sd(cfg, 42))
    g = torch.Generator().manual_seed(43)
    xs = {R: torch.randn(R, H, generator=g).bfloat16().to(dev) for R in ROWS}
    out = {"x": xs, "w8": {}, "w8_again": {}, "pair": {}, "bf16": {}}
    try:
        q = _engine(cfg, sd, FP8, max_batch=8)
        es = [q.w[f"lm.{l}.{n}{W8_EXPS}"] for l in range(2) for n in ("gu_w", "down_w")]
        out["exps"] = [int(e.to(torch.int32).max() - e.to(torch.int32).min()) for e in es]
        for R in ROWS:
            assert L.vv_lm_ffn_active(q.h, R) == 1, R
            out["w8"][R] = _replay(q, xs[R])
            out["w8_again"][R] = _replay(q, xs[R])
        L.vv_lm_ffn_w8(0)
        for R in ROWS:
            assert L.vv_lm_ffn_active(q.h, R) == 0, R
            out["pair"][R] = _replay(q, xs[R])
        L.vv_lm_ffn_w8(3)
        q.check_sync()
        assert_counters_consistent(q)
        q.close()
        del q
        gc.collect()
        b = _engine(cfg, fake_quantize_state_dict(sd, cfg), None, max_batch=8)
        assert not b.weights_quantized()
        for R in ROWS:
            assert L.vv_lm_ffn_active(b.h, R) == 1, R
            out["bf16"][R] = _replay(b, xs[R])
        b.check_sync()
        b.close()
    finally:
        L.vv_lm_ffn_w8(3)
    return out


def test_exponents_differ_widely(blocks):
    assert all(s >= 12 for s in blocks["exps"]), blocks["exps"]


@pytest.mark.parametrize("R", ROWS)
def test_bit_identical_to_bf16_on_dequantised(blocks, R):
    w8, again, ref = blocks["w8"][R], blocks["w8_again"][R], blocks["bf16"][R]
    assert torch.isfinite(w8.float()).all() and not torch.equal(w8, blocks["x"][R])
    assert torch.equal(w8.view(torch.int16), again.view(torch.int16))
    diff = (w8.view(torch.int16) != ref.view(torch.int16)).sum().item()
    print(f"R={R}: {diff} of {w8.numel()} outputs differ from the bf16 kernel on the dequantised weights")
    assert torch.equal(w8.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("R", ROWS)
def test_within_bf16_of_the_gemv_pair(blocks, R):
    one, pair = blocks["w8"][R], blocks["pair"][R]
    print(f"R={R}: one launch vs the FP8 GEMV pair: rel {rel_err(one, pair):.3e} cosine {cos(one, pair):.6f}")
    assert rel_err(one, pair) < 2e-2 and cos(one, pair) > 0.999


# ------------------------------------------------------------------ 3. decode against the oracle
@pytest.mark.parametrize("n", [1, 3])
def test_decode_vs_oracle(n):
    L = _lib.lib()
    cfg = _cfg()
    sd = _sd(cfg, 44 + n)
    eng = _engine(cfg, sd, FP8, max_batch=n, max_ctx=256)
    R = 2 * n
    assert L.vv_lm_ffn_active(eng.h, R) == 1 and L.vv_lm_attn_active(eng.h, R, 64) == 0
    lcfg = dict(cfg.decoder_config)
    osd = _oracle_sd(fake_quantize_state_dict(sd, cfg))
    g = torch.Generator().manual_seed(50 + n)
    lens = [5 + 3 * r for r in range(R)]
    xs = [torch.randn(m, H, generator=g).bfloat16() for m in lens]
    kvs = [olm.RowKV(2) for _ in lens]
    for r in range(R):
        olm.forward_rows(osd, lcfg, xs[r][None], kvs[r:r + 1])
    slots = torch.cat([torch.full((m,), r) for r, m in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(m) for m in lens]).to(**I32)
    last = torch.cumsum(torch.tensor(lens), 0) - 1
    eng.lm_forward(torch.cat(xs).to(dev), slots, pos, last.to(**I32))
    Lt = torch.tensor(lens)
    for s in range(3):
        step_x = torch.randn(R, H, generator=g).bfloat16()
        ref = olm.forward_rows(osd, lcfg, step_x[:, None], kvs)[:, -1]
        h, _ = eng.lm_forward(step_x.to(dev), torch.arange(R).to(**I32), Lt.to(**I32), torch.arange(R).to(**I32))
        torch.cuda.synchronize()
        Lt += 1
        print(f"n={n} step {s}: rel {rel_err(h, ref):.3e} cosine {cos(h, ref):.6f} vs the oracle")
        assert rel_err(h, ref) < 2e-2 and cos(h, ref) > 0.999
    eng.check_sync()
    assert_counters_consistent(eng)
    eng.close()


# ------------------------------------------------------------------ 4. graphs
def test_graphs_and_switch_recapture():
    L = _lib.lib()
    cfg = _cfg()
    m = VibeVoiceForConditionalGenerationInference(cfg, _sd(cfg, 48), dev, max_batch=1, max_ctx=256, weight_dtype=FP8)
    m.set_ddpm_inference_steps(5)
    assert L.vv_weights_quantized(m.engine.h) == 1 and L.vv_lm_ffn_active(m.engine.h, 2) == 1
    ids = torch.randint(0, 151000, (1, 12), generator=torch.Generator().manual_seed(3))
    mask = torch.ones(1, 12, dtype=torch.long)
    sched = [[D, D, D, E, S, D, X]]

    def run(graphs):
        torch.manual_seed(77)
        o = m.generate(input_ids=ids, attention_mask=mask, tokenizer=TK, cfg_scale=1.3, forced_tokens=sched,
                       use_graphs=graphs, show_progress_bar=False)
        return o.sequences.clone(), o.speech_outputs[0].clone()

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    eager, graph = run(False), run(True)
    assert len(m._graph_cache) >= 1 and torch.isfinite(eager[1].float()).all()
    assert same(eager, graph)
    e0 = m._graph_epoch
    L.vv_lm_ffn_w8(0)                                    # the GEMV pair: graphs of the other path must go
    assert L.vv_lm_ffn_active(m.engine.h, 2) == 0
    pair = run(True)
    assert m._graph_epoch != e0 and torch.isfinite(pair[1].float()).all()
    e1 = m._graph_epoch
    L.vv_lm_ffn_w8(3)
    assert L.vv_lm_ffn_active(m.engine.h, 2) == 1
    back = run(True)
    assert m._graph_epoch != e1
    assert same(back, graph)
    m.engine.check_sync()
    assert_counters_consistent(m.engine)
    m.engine.close()


# ------------------------------------------------------------------ 5. a mixed binding
def test_mixed_binding_keeps_the_gemv_pair():
    """One layer's down projection bound as bf16 (dequantised, MFMA-packed), every
    other projection as FP8, through Engine(packed=...): no one-launch block, and
    the decode step equals the same binding under vv_lm_ffn(0) bit for bit."""
    L = _lib.lib()
    cfg = _cfg()
    q = _engine(cfg, _sd(cfg, 49), FP8, max_batch=1)
    assert L.vv_lm_ffn_active(q.h, 2) == 1
    w = dict(q.w)
    q.close()
    del q
    gc.collect()
    codes, ex = w.pop("lm.1.down_w" + W8_CODES), w.pop("lm.1.down_w" + W8_EXPS)
    w["lm.1.down_w"] = mfma_pack(dequantize_rows(mfma_unpack8(codes), ex)).contiguous()
    eng = Engine(cfg, None, dev, max_batch=1, max_ctx=128, valid_ids=VALID, packed=w)
    assert eng.weights_quantized()
    assert [L.vv_lm_ffn_active(eng.h, r) for r in (1, 2)] == [0, 0]
    g = torch.Generator().manual_seed(51)
    lens = [7, 4]
    x = torch.randn(sum(lens), H, generator=g).bfloat16().to(dev)
    slots = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(n) for n in lens]).to(**I32)
    eng.lm_forward(x, slots, pos, torch.tensor([lens[0] - 1, sum(lens) - 1]).to(**I32))
    step_x = torch.randn(2, H, generator=g).bfloat16().to(dev)
    outs = []
    for on in (1, 0):
        L.vv_lm_ffn(on)
        h, lg = eng.lm_forward(step_x, torch.arange(2).to(**I32), torch.tensor(lens).to(**I32), torch.arange(2).to(**I32))
        torch.cuda.synchronize()
        outs.append((h.clone(), lg.clone()))
    L.vv_lm_ffn(1)
    assert torch.isfinite(outs[0][0].float()).all()
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1], outs[1][1])
    eng.check_sync()
    eng.close()
