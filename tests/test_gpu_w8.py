"""FP8 (OCP e4m3fn) weight-only storage of the LM projections on the GPU.

An e4m3 code times a power of two is exact in bf16, so an engine holding FP8
weights computes the products of a bf16 engine holding the dequantised weights;
only the fp32 summation order may differ.  Hence:

* the FP8 GEMV (csrc/gemv_w8.hip, vv_gemm_w8) is held to test_gpu_gemm.py's own
  bounds against the fp32 product with the dequantised matrix;
* the fallback (more than 16 rows, or vv_gemv_w8(0)) is bit-identical to a bf16
  engine built from fake_quantize_state_dict;
* the decode loop is held to DESIGN.md §4's bounds against the oracle run on the
  fake-quantised state dict.
"""
import ctypes
import functools
import gc

import pytest
import torch

from gpu_util import kv_synthetic, max_rel, rel_err
from teacher import oracle_run, per_step_check, teacher_forced
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.synthetic import synthetic_inputs, tokenizer_ids
from vibevoice_amd.weights import (LM_QUANTIZED, W8_CODES, W8_EXPS, dequantize_rows, fake_quantize_state_dict,
                                   mfma_pack8, quantize_rows_e4m3, synthetic_state_dict, write_synthetic_checkpoint)

pytestmark = pytest.mark.gpu
dev = "cuda"
I32 = dict(dtype=torch.int32, device=dev)
TK = tokenizer_ids()
IDS = dict(eos=TK.eos_token_id, start=TK.speech_start_id, end=TK.speech_end_id, diffusion=TK.speech_diffusion_id)
D, E, S, X = IDS["diffusion"], IDS["end"], IDS["start"], IDS["eos"]
VALID = [151643, 151652, 151653, 151654]
FP8 = "fp8_e4m3"


@pytest.fixture(autouse=True)
def _collect_engines():
    gc.collect()
    yield
    _lib.lib().vv_gemv_w8(1)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------ the kernel
@functools.lru_cache(maxsize=None)
def _weight(N, K):
    """Rows scaled by 2^-12 .. 2^6 (distinct exponents per row of a tile), row 3
    all zero -> (dequantised bf16 [N, K], packed codes, exponents)."""
    g = torch.Generator(device=dev).manual_seed(N * 3 + K)
    W = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
    ex = torch.arange(N, device=dev) % 19 - 12
    W = torch.ldexp(W, ex[:, None]).bfloat16()
    W[3] = 0
    codes, e = quantize_rows_e4m3(W)
    assert e[3] == 0 and e.unique().numel() >= 12
    return dequantize_rows(codes, e), mfma_pack8(codes).contiguous(), e.contiguous()


def run(M, N, K, epi="store", xf=0, norm_w=False, bias=False, res=False, twice=True):
    Wd, codes, e = _weight(N, K)
    g = torch.Generator(device=dev).manual_seed(M * 7 + N + K)
    A = torch.randn(M, K, device=dev, generator=g).bfloat16()
    b = (0.1 * torch.randn(N, device=dev, generator=g)).bfloat16() if bias else None
    nw = (1.0 + 0.1 * torch.randn(K, device=dev, generator=g)).bfloat16() if norm_w else None
    outN = N // 2 if epi == "silu_mul" else N
    R = torch.randn(M, outN, device=dev, generator=g).bfloat16() if res else None
    eps = 1e-6
    ys = []
    for _ in range(2 if twice else 1):
        Y = torch.full((M, outN), float("nan"), device=dev, dtype=torch.bfloat16)
        rc = _lib.lib().vv_gemm_w8(M, N, K, P(A), K, P(codes), P(e), xf, P(nw), eps, P(b), _lib.EPI[epi], P(Y), outN,
                                   P(R), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "gemm_w8")
        torch.cuda.synchronize()
        ys.append(Y)
    if twice:
        assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16))      # deterministic
    Af = A.float()
    if xf == 1:
        x = (Af * torch.rsqrt(Af.pow(2).mean(-1, keepdim=True) + eps)).bfloat16()
        if nw is not None:
            x = (x.float() * nw.float()).bfloat16()
        Af = x.float()
    acc = Af @ Wd.float().t()
    if b is not None:
        acc = acc + b.float()
    if epi == "store":
        ref = acc.bfloat16()
    elif epi == "silu_mul":
        a = acc.view(M, N // 16, 2, 8)
        gate, up = a[:, :, 0].reshape(M, N // 2), a[:, :, 1].reshape(M, N // 2)
        ref = (torch.nn.functional.silu(gate.bfloat16().float()).bfloat16().float() * up.bfloat16().float()).bfloat16()
    else:
        ref = (R.float() + acc.bfloat16().float()).bfloat16()
    return ys[0], ref, e


def check(Y, ref, tag, e=None):
    r, m = rel_err(Y, ref), max_rel(Y, ref)
    print(f"{tag}: rel L2 {r:.3e} max-rel {m:.3e}")
    assert r < 4e-3 and m < 3e-2, (tag, r, m)
    if e is not None:
        # per output column at its own scale (exact power-of-two rescale): a wrong
        # row <-> exponent mapping in the small-scale rows cannot hide behind the large ones
        s = -e.to(torch.int32)[None, :]
        Yn, rn = torch.ldexp(Y.float(), s), torch.ldexp(ref.float(), s)
        r, m = rel_err(Yn, rn), max_rel(Yn, rn)
        print(f"{tag} (per-row scale removed): rel L2 {r:.3e} max-rel {m:.3e}")
        assert r < 4e-3 and m < 3e-2, (tag, r, m)
        assert torch.equal(Y[:, 3], ref[:, 3])                 # the all-zero row: exactly the bias (or 0)


@pytest.mark.parametrize("M", [1, 2, 5, 16])
@pytest.mark.parametrize("N", [16, 48, 4608])
@pytest.mark.parametrize("K", [64, 192, 3584])
def test_gemv_w8_store(M, N, K):
    Y, ref, e = run(M, N, K)
    check(Y, ref, f"w8 store M={M} N={N} K={K}", e)


@pytest.mark.parametrize("M", [2, 16])
@pytest.mark.parametrize("case", ["bias", "res", "silu_mul", "norm", "norm_w", "rope_like_bias_norm"])
def test_gemv_w8_forms(M, case):
    N, K = 48, 192
    kw = dict(bias=dict(bias=True), res=dict(epi="res", res=True), silu_mul=dict(epi="silu_mul"),
              norm=dict(xf=1), norm_w=dict(xf=1, norm_w=True),
              rope_like_bias_norm=dict(xf=1, norm_w=True, bias=True))[case]
    Y, ref, e = run(M, N, K, **kw)
    check(Y, ref, f"w8 {case} M={M}", e if kw.get("epi", "store") == "store" else None)


def test_gemv_w8_k_blocks_and_large_width():
    """16 rows of K = 18,944 exceed the LDS budget: the A rows are staged in K
    blocks (the Large down projection at B = 8); N = 3,584 as there."""
    Y, ref, e = run(16, 64, 18944, twice=False)
    check(Y, ref, "w8 store M=16 N=64 K=18944 (K blocks)", e)
    Y, ref, e = run(2, 64, 18944, epi="res", res=True, twice=False)
    check(Y, ref, "w8 res M=2 N=64 K=18944")


def test_gemv_w8_switch_and_more_rows_equal_bf16_on_dequantised():
    """vv_gemv_w8(0) and M > 16: dequantise + the bf16 kernels, bit for bit
    vv_gemm_bf16 on the dequantised matrix."""
    from vibevoice_amd.weights import mfma_pack
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for M, off in ((2, True), (40, False)):
        N, K = 48, 192
        Wd, codes, e = _weight(N, K)
        A = torch.randn(M, K, device=dev, generator=torch.Generator(device=dev).manual_seed(M)).bfloat16()
        Y8 = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        Yb = torch.empty_like(Y8)
        L.vv_gemv_w8(0 if off else 1)
        _lib.check(L.vv_gemm_w8(M, N, K, P(A), K, P(codes), P(e), 0, None, 0.0, None, 0, P(Y8), N, None, None, st), "w8")
        L.vv_gemv_w8(1)
        _lib.check(L.vv_gemm_bf16(M, N, K, P(A), K, P(mfma_pack(Wd)), None, 0, P(Yb), N, None, None, None, st), "bf16")
        torch.cuda.synchronize()
        assert torch.equal(Y8.view(torch.int16), Yb.view(torch.int16)), M


# ------------------------------------------------------------------ engines
def _sd(cfg, seed):
    return synthetic_state_dict(cfg, seed=seed, device="cpu", mode="test", with_acoustic_encoder=False)


def _pair(cfg, seed, max_batch=2, max_ctx=128):
    """(FP8 engine, bf16 engine on the fake-quantised state dict), both on the
    per-op kernels (the one-launch LM kernels read bf16 weights)."""
    sd = _sd(cfg, seed)
    q = Engine(cfg, sd, dev, max_batch=max_batch, max_ctx=max_ctx, valid_ids=VALID, persistent=False,
               weight_dtype=FP8)
    b = Engine(cfg, fake_quantize_state_dict(sd, cfg), dev, max_batch=max_batch, max_ctx=max_ctx, valid_ids=VALID,
               persistent=False)
    assert q.weight_dtype == FP8 and b.weight_dtype is None
    assert q.weights_quantized() and not b.weights_quantized()
    return q, b


def test_fallback_is_bit_identical_to_bf16_on_dequantised():
    cfg = tiny_config()
    q, b = _pair(cfg, seed=21)
    H = cfg.decoder_config.hidden_size
    g = torch.Generator().manual_seed(1)
    x = torch.randn(40, H, generator=g).bfloat16().to(dev)            # 40 prompt rows of slot 0 (> 16)
    slots, pos = torch.zeros(40, **I32), torch.arange(40, **I32)
    out_idx = torch.tensor([39], **I32)
    hq, lq = q.lm_forward(x, slots, pos, out_idx)
    hb, lb = b.lm_forward(x, slots, pos, out_idx)
    torch.cuda.synchronize()
    assert torch.isfinite(hq.float()).all()
    assert torch.equal(hq.view(torch.int16), hb.view(torch.int16)) and torch.equal(lq, lb)
    # decode rows on the fallback read that KV: equal again only if the cache is
    _lib.lib().vv_gemv_w8(0)
    for s in range(2):
        xs = torch.randn(1, H, generator=g).bfloat16().to(dev)
        args = (xs, torch.zeros(1, **I32), torch.tensor([40 + s], **I32), torch.zeros(1, **I32))
        hq, lq = q.lm_forward(*args)
        hb, lb = b.lm_forward(*args)
        torch.cuda.synchronize()
        assert torch.equal(hq.view(torch.int16), hb.view(torch.int16)) and torch.equal(lq, lb), s
    _lib.lib().vv_gemv_w8(1)
    # and the FP8 GEMV on the same cache stays within the LM bound of the bf16 engine
    xs = torch.randn(1, H, generator=g).bfloat16().to(dev)
    args = (xs, torch.zeros(1, **I32), torch.tensor([42], **I32), torch.zeros(1, **I32))
    hq, _ = q.lm_forward(*args)
    hb, _ = b.lm_forward(*args)
    torch.cuda.synchronize()
    print("decode row, FP8 GEMV vs bf16 on dequantised: rel", rel_err(hq, hb))
    assert rel_err(hq, hb) < 2e-2


def _ulps(a, b):
    def key(t):
        i = t.contiguous().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs().max().item()


def test_rope_kv_epilogue_real_head_shape():
    """One layer, 2 q heads / 1 kv head of 128 (hidden 256), rows at positions
    {0, 1, 37}: q and the K / V cache of the FP8 GEMV vs the bf16 engine on the
    dequantised weights, within 1 bf16 ulp elementwise (summation order only)."""
    cfg = tiny_config(hidden=256, layers=1, heads=2, kv_heads=1, inter=512)
    q, b = _pair(cfg, seed=22)
    slots_h, pos_h = [0, 1, 2], [0, 1, 37]
    slots, pos = torch.tensor(slots_h, **I32), torch.tensor(pos_h, **I32)
    x = torch.randn(3, 256, generator=torch.Generator().manual_seed(2)).bfloat16().to(dev)
    got = []
    for eng in (q, b):
        kv_synthetic(eng, slots, 0, 38, seed=5)
        eng.lm_forward(x, slots, pos, torch.arange(3, **I32), max_pos=37)
        qo = torch.empty(3, 2 * 128, device=dev, dtype=torch.bfloat16)
        ko, vo = (torch.empty(3, 1, 128, device=dev, dtype=torch.bfloat16) for _ in range(2))
        arr = ctypes.c_int * 3
        _lib.check(_lib.lib().vv_diag_lm_qkv(eng.h, 3, 0, arr(*slots_h), arr(*pos_h), P(qo), P(ko), P(vo)), "diag_lm_qkv")
        torch.cuda.synchronize()
        got.append((qo.cpu(), ko.cpu(), vo.cpu()))
    for name, a, r in zip("qkv", got[0], got[1]):
        assert torch.isfinite(a.float()).all() and a.float().abs().max() > 0
        u = _ulps(a, r)
        print(f"{name}: max |ulp| difference {u}, rel L2 {rel_err(a, r):.3e}")
    for name, a, r in zip("qkv", got[0], got[1]):
        assert _ulps(a, r) <= 1, name


# ------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def tiny_fp8():
    cfg = tiny_config()
    sd = _sd(cfg, 23)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, dev, max_batch=4, max_ctx=256, weight_dtype=FP8)
    m.set_ddpm_inference_steps(5)
    yield cfg, sd, m
    m.engine.close()


@pytest.mark.parametrize("B", [1, 3])
def test_decode_vs_oracle_on_fake_quantised(tiny_fp8, B):
    cfg, sd, m = tiny_fp8
    L = _lib.lib()
    assert L.vv_weights_quantized(m.engine.h) == 1
    assert L.vv_lm_ffn_active(m.engine.h, 2 * B) == 0 and L.vv_lm_attn_active(m.engine.h, 2 * B, 64) == 0
    inp = synthetic_inputs(batch=B, speakers=1, voice_seconds=0, text_tokens=8, seed=30 + B, hop=cfg.hop)
    sched = [[D] * 4 + [E, S, D, X]] if B == 1 else [[D, D, D, X], [D, E, S, D, X], [S, D, D, X]]
    fsd = fake_quantize_state_dict(sd, cfg)
    rec, seqs, _, _ = oracle_run(fsd, cfg, inp, sched, IDS, 5, None, 1234)
    got, sess = teacher_forced(m, inp, sched, rec, TK, 1234)
    assert torch.equal(sess.result().sequences, seqs)
    per_step_check(got, rec, None, f"tiny FP8 B={B}")


def test_default_engine_is_not_quantised():
    cfg = tiny_config()
    eng = Engine(cfg, _sd(cfg, 24), dev, max_batch=1, max_ctx=64)
    assert _lib.lib().vv_weights_quantized(eng.h) == 0 and eng.weight_dtype is None
    assert all(v.dtype != torch.float8_e4m3fn for v in eng.w.values())
    eng.close()


def test_finalize_names_half_bound_pair(tiny_fp8):
    cfg, _, m = tiny_fp8
    w = dict(m.engine.w)
    del w["lm.1.o_w" + W8_EXPS]
    with pytest.raises(RuntimeError, match="lm.1.o_we"):
        Engine(cfg, None, dev, max_batch=1, max_ctx=64, packed=w, persistent=False)
    w = dict(m.engine.w)
    del w["lm.0.gu_w" + W8_CODES], w["lm.0.gu_w" + W8_EXPS]
    with pytest.raises(RuntimeError, match="lm.0.gu_w"):
        Engine(cfg, None, dev, max_batch=1, max_ctx=64, packed=w, persistent=False)


def test_graph_replay_matches_eager_fp8(tiny_fp8):
    cfg, sd, m = tiny_fp8
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 151000, (2, 12), generator=g)
    mask = torch.ones(2, 12, dtype=torch.long)
    sched = [[D] * 3 + [E, S] + [D] * 3 + [X], [D] * 2 + [S] + [D] * 5 + [X]]          # 8 steps
    outs = []
    for graphs in (False, True):
        torch.manual_seed(77)
        outs.append(m.generate(input_ids=ids, attention_mask=mask, tokenizer=TK, cfg_scale=1.3, forced_tokens=sched,
                               use_graphs=graphs, show_progress_bar=False))
    assert len(m._graph_cache) >= 1
    assert torch.equal(outs[0].sequences, outs[1].sequences)
    for b in range(2):
        a0, a1 = outs[0].speech_outputs[b].cpu(), outs[1].speech_outputs[b].cpu()
        assert torch.isfinite(a0.float()).all() and torch.equal(a0, a1)


# ------------------------------------------------------------------ public interface
def test_from_pretrained_weight_dtype(tmp_path):
    """Fails on a build without the feature: unknown keyword."""
    cfg = tiny_config(hidden=256, layers=2, heads=2, kv_heads=1, inter=512)
    write_synthetic_checkpoint(str(tmp_path), cfg, seed=9, mode="test")
    m = VibeVoiceForConditionalGenerationInference.from_pretrained(str(tmp_path), torch_dtype=torch.bfloat16,
                                                                   device_map="cuda", max_batch=2, max_ctx=128,
                                                                   weight_dtype=FP8)
    assert m.weight_dtype == FP8 and m.engine.weight_dtype == FP8 and m.engine.weights_quantized()
    for l in range(2):
        for n in LM_QUANTIZED:
            k = f"lm.{l}.{n}"
            assert k not in m.engine.w
            assert m.engine.w[k + W8_CODES].dtype in (torch.float8_e4m3fn, torch.uint8)
            assert m.engine.w[k + W8_EXPS].dtype == torch.int8
    m.set_ddpm_inference_steps(3)
    ids = torch.randint(0, 151000, (1, 12), generator=torch.Generator().manual_seed(4))
    torch.manual_seed(5)
    out = m.generate(input_ids=ids, attention_mask=torch.ones(1, 12, dtype=torch.long), tokenizer=TK, cfg_scale=1.3,
                     forced_tokens=[[D, D, D, D, X]], show_progress_bar=False)
    audio = out.speech_outputs[0].float().cpu()
    assert audio.shape[-1] == 4 * m.engine.hop and torch.isfinite(audio).all() and audio.abs().max() > 0
    with pytest.raises(ValueError, match="fp8_e4m3"):
        VibeVoiceForConditionalGenerationInference.from_pretrained(str(tmp_path), weight_dtype="int4")
