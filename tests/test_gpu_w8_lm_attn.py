"""The one-launch LM attention kernel on FP8 weights (lm_attn.hip: k_lm_attn's W8
form, the per-engine option lm_attn_w8 / vv_set_lm_attn_w8, default off).

The W8 form keeps the bf16 form's workgroup roles, k-block ranges, MFMA order,
LDS sums, epilogues, attention phases and waits, and converts a weight fragment
to code * 2^e[row] -- exactly the bf16 value -- where the bf16 form reads its
register.  So an FP8 engine's decode step must equal, bit for bit, that of a
bf16 engine built from fake_quantize_state_dict (every other kernel of the two
engines is pinned to that by the suite already).  Against the FP8 GEMVs + k_attn
(another summation order) and the oracle the bound is test_gpu_lm.py's for the
one launch against the three: rel L2 < 2e-2, cosine > 0.999.

All engines are the smallest the kernel accepts (H 1536, 12 / 2 heads, I 8960, 2
layers so the per-layer weight table is exercised), built one after another: a
one-launch kernel runs only while its context is the device's only registered one.
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
H, I, NH, NKV, HD = 1536, 8960, 12, 2, 128
LMP = "model.language_model."
MAX_CTX = 256


@pytest.fixture(autouse=True)
def _switches():
    gc.collect()
    yield
    _lib.lib().vv_lm_attn(1)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def _cfg():
    return tiny_config(hidden=H, layers=2, heads=NH, kv_heads=NKV, inter=I)


def _sd(cfg, seed):
    return synthetic_state_dict(cfg, seed=seed, device="cpu", mode="test", with_acoustic_encoder=False)


def _engine(cfg, sd, weight_dtype, max_batch, lm_attn_w8=False):
    return Engine(cfg, sd, dev, max_batch=max_batch, max_ctx=MAX_CTX, valid_ids=VALID, weight_dtype=weight_dtype,
                  lm_attn_w8=lm_attn_w8)


def _oracle_sd(sd):
    return {k[len(LMP):]: v for k, v in sd.items() if k.startswith(LMP)}


# ------------------------------------------------------------------ 1. which path runs
def test_active():
    cfg = _cfg()
    sd = _sd(cfg, 61)
    L = _lib.lib()
    rows = (1, 2, 3, 16, 17)
    act = lambda e: [L.vv_lm_attn_active(e.h, r, 64) for r in rows]   # noqa: E731
    q = _engine(cfg, sd, FP8, max_batch=8, lm_attn_w8=True)
    assert q.weights_quantized() and L.vv_lm_attn_w8(q.h) == 1
    assert act(q) == [1, 1, 1, 1, 0]
    L.vv_lm_attn(0)
    assert act(q) == [0, 0, 0, 0, 0]
    L.vv_lm_attn(1)
    assert act(q) == [1, 1, 1, 1, 0]
    assert L.vv_set_lm_attn_w8(q.h, 0) != 0 and b"vv_set_lm_attn_w8" in L.vv_last_error()   # after finalize
    assert L.vv_lm_attn_w8(q.h) == 1
    q.close()
    del q
    gc.collect()
    off = _engine(cfg, sd, FP8, max_batch=8)               # the same engine without the option: the three launches
    assert off.weights_quantized() and L.vv_lm_attn_w8(off.h) == 0
    assert act(off) == [0, 0, 0, 0, 0]
    off.close()
    del off
    gc.collect()
    b = _engine(cfg, sd, None, max_batch=8)                # a bf16 engine: as before
    assert L.vv_lm_attn_w8(b.h) == 0 and act(b) == [1, 1, 1, 1, 0]
    L.vv_lm_attn(0)
    assert act(b) == [0, 0, 0, 0, 0]
    L.vv_lm_attn(1)
    assert act(b) == [1, 1, 1, 1, 0]
    b.close()


# ------------------------------------------------------------------ 2. bit identity
ROWS = (1, 2, 3, 6, 16)
LENS = (1, 31, 32, 33, 64, 200)     # per-row context lengths, cycled: both sides of the 32-key unit edges
V0 = (NH + NKV) * HD                # first v row of the packed q|k|v matrix


def _spread_exponents(cfg, sd):
    """Row n of every layer's v_proj and o_proj times 2^((n mod 13) - 6): the rows of
    one 16-row tile get widely different exponents.  q_proj and k_proj rows times
    2^((n mod 3) - 1) only, so that the softmax is not driven one-hot and the
    attention phases stay sensitive.  A power of two commutes with the quantiser, so
    the FP8 and the fake-quantised engines still hold equal values.  One v row and
    one o row per layer are zero (exponent 0)."""
    def scaled(w, e):
        return torch.ldexp(w.float(), e[:, None].to(torch.int32)).to(w.dtype)
    for l in range(cfg.decoder_config.num_hidden_layers):
        p = f"{LMP}layers.{l}.self_attn."
        q, k, v, o = (sd[p + n + "_proj.weight"] for n in "qkvo")
        q, k = scaled(q, torch.arange(q.shape[0]) % 3 - 1), scaled(k, torch.arange(k.shape[0]) % 3 - 1)
        v, o = scaled(v, torch.arange(v.shape[0]) % 13 - 6), scaled(o, torch.arange(o.shape[0]) % 13 - 6)
        v[37 + 16 * l] = 0
        o[21 + 16 * l] = 0
        for n, w in zip("qkvo", (q, k, v, o)):
            sd[p + n + "_proj.weight"] = w
    return sd


def _lens(R):
    return [LENS[r % len(LENS)] for r in range(R)]


def _kv_last(eng, lens, ahead):
    """The K and V rows (both layers) each row appended last: position lens[r] + ahead of slot r."""
    ks, vs = [], []
    for r, n in enumerate(lens):
        k = torch.empty(2, NKV, 1, HD, dtype=torch.bfloat16, device=dev)
        v = torch.empty_like(k)
        _lib.check(_lib.lib().vv_diag_kv_read(eng.h, r, n + ahead, n + ahead + 1, P(k), P(v)), "diag_kv_read")
        ks.append(k)
        vs.append(v)
    return torch.stack(ks).view(torch.int16).cpu(), torch.stack(vs).view(torch.int16).cpu()


def _decode(eng, xs, R, extra):
    """Prefill the R rows, then 2 decode steps; (hidden bits, logits) per step, the rows
    appended by step 2, and with `extra` step 2 again as it is and under vv_lm_attn(15)."""
    L = _lib.lib()
    lens = _lens(R)
    slots = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(n) for n in lens]).to(**I32)
    last = (torch.cumsum(torch.tensor(lens), 0) - 1).to(**I32)
    eng.lm_forward(xs["prefill"], slots, pos, last)
    ar = torch.arange(R).to(**I32)

    def step(s):
        assert L.vv_lm_attn_active(eng.h, R, max(lens) + s + 1) == 1, (R, s)
        h, lg = eng.lm_forward(xs["step"][s], ar, (torch.tensor(lens) + s).to(**I32), ar)
        torch.cuda.synchronize()
        return h.view(torch.int16).cpu(), lg.cpu()

    out = {"steps": [step(0), step(1)], "kv": _kv_last(eng, lens, 1)}
    if extra:
        out["again"] = step(1)
        L.vv_lm_attn(15)      # every A/B bit cleared: the kernel's first form (LmAttnArgs::variant 0)
        out["first_form"] = step(1)
        L.vv_lm_attn(1)
        out["kv_first_form"] = _kv_last(eng, lens, 1)
    return out


@pytest.fixture(scope="module")
def runs():
    """{R: operands}, the FP8 engine's decode steps with the option on and the bf16
    engine's on the fake-quantised weights; computed once."""
    gc.collect()
    L = _lib.lib()
    cfg = _cfg()
    sd = _spread_exponents(cfg, _sd(cfg, 62))
    g = torch.Generator().manual_seed(63)
    xs = {R: {"prefill": torch.randn(sum(_lens(R)), H, generator=g).bfloat16().to(dev),
              "step": [torch.randn(R, H, generator=g).bfloat16().to(dev) for _ in range(2)]} for R in ROWS}
    out = {"w8": {}, "bf16": {}}
    try:
        q = _engine(cfg, sd, FP8, max_batch=8, lm_attn_w8=True)
        span = lambda e: int(e.to(torch.int32).max() - e.to(torch.int32).min())   # noqa: E731
        out["exps"] = [span(q.w[f"lm.{l}.qkv_w{W8_EXPS}"][V0:]) for l in range(2)] + \
                      [span(q.w[f"lm.{l}.o_w{W8_EXPS}"]) for l in range(2)]
        for R in ROWS:
            out["w8"][R] = _decode(q, xs[R], R, True)
        q.check_sync()
        assert_counters_consistent(q)
        q.close()
        del q
        gc.collect()
        b = _engine(cfg, fake_quantize_state_dict(sd, cfg), None, max_batch=8)
        assert not b.weights_quantized()
        for R in ROWS:
            out["bf16"][R] = _decode(b, xs[R], R, False)
        b.check_sync()
        b.close()
    finally:
        L.vv_lm_attn(1)
    return out


def test_exponents_differ_widely(runs):
    assert all(s >= 12 for s in runs["exps"]), runs["exps"]


@pytest.mark.parametrize("R", ROWS)
def test_bit_identical_to_bf16_on_dequantised(runs, R):
    w8, ref = runs["w8"][R], runs["bf16"][R]
    for s in range(2):
        (h, lg), (hr, lgr) = w8["steps"][s], ref["steps"][s]
        assert torch.isfinite(lg).all() and torch.isfinite(h.view(torch.bfloat16).float()).all()
        diff = (h != hr).sum().item()
        print(f"R={R} step {s}: {diff} of {h.numel()} hidden values differ from the bf16 kernel on the dequantised weights")
        assert torch.equal(h, hr) and torch.equal(lg, lgr)
    for name, a, b in zip("KV", w8["kv"], ref["kv"]):
        print(f"R={R}: {(a != b).sum().item()} of {a.numel()} appended {name} values differ")
        assert a.any() and torch.equal(a, b)
    h, lg = w8["steps"][1]
    for other in ("again", "first_form"):
        assert torch.equal(w8[other][0], h) and torch.equal(w8[other][1], lg), other
    assert all(torch.equal(a, b) for a, b in zip(w8["kv_first_form"], w8["kv"]))


# ------------------------------------------------------------------ 3. against the other paths
@pytest.mark.parametrize("n", [1, 3])
def test_decode_vs_three_launches_and_oracle(n):
    L = _lib.lib()
    cfg = _cfg()
    sd = _sd(cfg, 64 + n)
    eng = _engine(cfg, sd, FP8, max_batch=n, lm_attn_w8=True)
    R = 2 * n
    assert L.vv_lm_attn_active(eng.h, R, 64) == 1
    lcfg = dict(cfg.decoder_config)
    osd = _oracle_sd(fake_quantize_state_dict(sd, cfg))
    g = torch.Generator().manual_seed(70 + n)
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
    ar = torch.arange(R).to(**I32)
    for s in range(3):
        step_x = torch.randn(R, H, generator=g).bfloat16()
        ref = olm.forward_rows(osd, lcfg, step_x[:, None], kvs)[:, -1]
        L.vv_lm_attn(0)           # the FP8 GEMVs + k_attn on the same KV state (the step's own rows are rewritten below)
        assert L.vv_lm_attn_active(eng.h, R, int(Lt.max()) + 1) == 0
        three, _ = eng.lm_forward(step_x.to(dev), ar, Lt.to(**I32), ar)
        torch.cuda.synchronize()
        three = three.clone()
        L.vv_lm_attn(1)
        assert L.vv_lm_attn_active(eng.h, R, int(Lt.max()) + 1) == 1
        one, _ = eng.lm_forward(step_x.to(dev), ar, Lt.to(**I32), ar)
        torch.cuda.synchronize()
        Lt += 1
        print(f"n={n} step {s}: one launch vs the three: rel {rel_err(one, three):.3e} cosine {cos(one, three):.6f}; "
              f"vs the oracle: rel {rel_err(one, ref):.3e} cosine {cos(one, ref):.6f}")
        assert rel_err(one, three) < 2e-2 and cos(one, three) > 0.999
        assert rel_err(one, ref) < 2e-2 and cos(one, ref) > 0.999
    eng.check_sync()
    assert_counters_consistent(eng)
    eng.close()


# ------------------------------------------------------------------ 4. graphs
def test_graphs():
    L = _lib.lib()
    cfg = _cfg()
    m = VibeVoiceForConditionalGenerationInference(cfg, _sd(cfg, 68), dev, max_batch=1, max_ctx=MAX_CTX,
                                                   weight_dtype=FP8, lm_attn_w8=True)
    m.set_ddpm_inference_steps(5)
    assert L.vv_weights_quantized(m.engine.h) == 1 and L.vv_lm_attn_w8(m.engine.h) == 1
    assert L.vv_lm_attn_active(m.engine.h, 2, 64) == 1
    ids = torch.randint(0, 151000, (1, 12), generator=torch.Generator().manual_seed(3))
    mask = torch.ones(1, 12, dtype=torch.long)
    sched = [[D, D, D, E, S, D, X]]

    def run(graphs):
        torch.manual_seed(77)
        o = m.generate(input_ids=ids, attention_mask=mask, tokenizer=TK, cfg_scale=1.3, forced_tokens=sched,
                       use_graphs=graphs, show_progress_bar=False)
        return o.sequences.clone(), o.speech_outputs[0].clone()

    eager, graph = run(False), run(True)
    assert len(m._graph_cache) >= 1 and torch.isfinite(eager[1].float()).all()
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    m.engine.check_sync()
    assert_counters_consistent(m.engine)
    m.engine.close()


# ------------------------------------------------------------------ 5. a mixed binding
def test_mixed_binding_keeps_the_three_launches():
    """One layer's o_proj bound as bf16 (dequantised, MFMA-packed), every other
    projection as FP8, through Engine(packed=...) with the option on: no one-launch
    attention, and the decode step equals the same binding under vv_lm_attn(0) bit
    for bit."""
    L = _lib.lib()
    cfg = _cfg()
    q = _engine(cfg, _sd(cfg, 69), FP8, max_batch=1, lm_attn_w8=True)
    assert L.vv_lm_attn_active(q.h, 2, 64) == 1
    w = dict(q.w)
    q.close()
    del q
    gc.collect()
    codes, ex = w.pop("lm.1.o_w" + W8_CODES), w.pop("lm.1.o_w" + W8_EXPS)
    w["lm.1.o_w"] = mfma_pack(dequantize_rows(mfma_unpack8(codes), ex)).contiguous()
    eng = Engine(cfg, None, dev, max_batch=1, max_ctx=MAX_CTX, valid_ids=VALID, packed=w, lm_attn_w8=True)
    assert eng.weights_quantized() and L.vv_lm_attn_w8(eng.h) == 1
    assert [L.vv_lm_attn_active(eng.h, r, 64) for r in (1, 2)] == [0, 0]
    g = torch.Generator().manual_seed(71)
    lens = [7, 4]
    x = torch.randn(sum(lens), H, generator=g).bfloat16().to(dev)
    slots = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(n) for n in lens]).to(**I32)
    eng.lm_forward(x, slots, pos, torch.tensor([lens[0] - 1, sum(lens) - 1]).to(**I32))
    step_x = torch.randn(2, H, generator=g).bfloat16().to(dev)
    outs = []
    for on in (1, 0):
        L.vv_lm_attn(on)
        h, lg = eng.lm_forward(step_x, torch.arange(2).to(**I32), torch.tensor(lens).to(**I32), torch.arange(2).to(**I32))
        torch.cuda.synchronize()
        outs.append((h.clone(), lg.clone()))
    L.vv_lm_attn(1)
    assert torch.isfinite(outs[0][0].float()).all()
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1], outs[1][1])
    eng.check_sync()
    eng.close()
