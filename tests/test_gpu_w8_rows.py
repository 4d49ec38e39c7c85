"""FP8 weight-only operands above 16 rows, read natively by the bf16 kernels.

k_gemv<2..4>, k_gemvw and k_gemm<64 / 32> have a W8 instantiation that loads
the e4m3 codes and converts them in registers to code * 2^e[n] -- the bf16 value
the dequantise pass would have stored -- ahead of the same MFMA sequence.  The
contract is bit identity with the bf16 kernel on the dequantised matrix (no
tolerance anywhere), with no k_dequant_w8 launch."""
import ctypes
import functools
import gc

import pytest
import torch

from teacher import oracle_run, per_step_check, teacher_forced
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.synthetic import synthetic_inputs, tokenizer_ids
from vibevoice_amd.weights import (dequantize_rows, fake_quantize_state_dict, mfma_pack, mfma_pack8,
                                   quantize_rows_e4m3, synthetic_state_dict)

pytestmark = pytest.mark.gpu
dev = "cuda"
I32 = dict(dtype=torch.int32, device=dev)
TK = tokenizer_ids()
IDS = dict(eos=TK.eos_token_id, start=TK.speech_start_id, end=TK.speech_end_id, diffusion=TK.speech_diffusion_id)
D, E, S, X = IDS["diffusion"], IDS["end"], IDS["start"], IDS["eos"]
VALID = [151643, 151652, 151653, 151654]
FP8 = "fp8_e4m3"
NATIVE = 1


@pytest.fixture(autouse=True)
def _collect_engines():
    gc.collect()
    yield
    _lib.lib().vv_gemv_w8(1)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def launches():
    return _lib.lib().vv_w8_dequant_launches()


# ------------------------------------------------------------------ the kernels
@functools.lru_cache(maxsize=None)
def _weight(N, K):
    """Rows scaled by 2^-12 .. 2^6 (distinct exponents per row of a tile); row 3
    all-zero codes; row 5 at exponent -20 and row 6 at -100 (the format's
    smallest), power-of-two scales far from 1 -> (dequantised bf16 [N, K] in
    mfma_pack order, packed codes, exponents)."""
    g = torch.Generator(device=dev).manual_seed(N * 3 + K)
    W = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
    ex = torch.arange(N, device=dev) % 19 - 12
    W = torch.ldexp(W, ex[:, None]).bfloat16()
    W[3] = 0
    codes, e = quantize_rows_e4m3(W)
    e[5], e[6] = -20, -100
    assert e[3] == 0 and not codes[3].float().any() and codes[5].float().abs().max() > 0
    Wd = dequantize_rows(codes, e)
    assert Wd[5].float().abs().max() < 2.0 ** -11 and Wd[6].float().abs().max() > 0
    return mfma_pack(Wd).contiguous(), mfma_pack8(codes).contiguous(), e.contiguous()


KINDS = dict(gemv=1, gemvw=2, gemm64=4, gemm32=5)


def run(M, N, K, kind, epi="store", xf=0, norm_w=False, bias=False, res=False, ksplit=None, mode=NATIVE):
    """vv_gemm_w8 twice and vv_gemm_bf16(_norm) on the dequantised matrix once:
    the three results bit-equal, no dequantise pass (mode NATIVE)."""
    L = _lib.lib()
    plan = (ctypes.c_int * 12)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert L.vv_gemm_plan_w8(M, N, K, xf, int(norm_w), 0, _lib.EPI[epi], 0, cus, plan, 12) == 0
    assert plan[0] == KINDS[kind] and plan[11] == mode, list(plan)
    if ksplit is not None:
        assert plan[3] == ksplit, list(plan)
    Wp, codes, e = _weight(N, K)
    g = torch.Generator(device=dev).manual_seed(M * 7 + N + K)
    A = torch.randn(M, K, device=dev, generator=g).bfloat16()
    b = (0.1 * torch.randn(N, device=dev, generator=g)).bfloat16() if bias else None
    nw = (1.0 + 0.1 * torch.randn(K, device=dev, generator=g)).bfloat16() if norm_w else None
    outN = N // 2 if epi == "silu_mul" else N
    R = torch.randn(M, outN, device=dev, generator=g).bfloat16() if res else None
    eps = 1e-6
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n0 = launches()
    ys = []
    for _ in range(2):
        Y = torch.full((M, outN), float("nan"), device=dev, dtype=torch.bfloat16)
        _lib.check(L.vv_gemm_w8(M, N, K, P(A), K, P(codes), P(e), xf, P(nw), eps, P(b), _lib.EPI[epi], P(Y), outN,
                                P(R), None, st), "gemm_w8")
        ys.append(Y)
    n1 = launches()
    Yb = torch.full((M, outN), float("nan"), device=dev, dtype=torch.bfloat16)
    if xf:
        assert b is None and R is None
        _lib.check(L.vv_gemm_bf16_norm(M, N, K, P(A), K, P(nw), eps, P(Wp), _lib.EPI[epi], P(Yb), outN, None, st), "bf16")
    else:
        _lib.check(L.vv_gemm_bf16(M, N, K, P(A), K, P(Wp), P(b), _lib.EPI[epi], P(Yb), outN, P(R), None, None, st), "bf16")
    torch.cuda.synchronize()
    assert torch.isfinite(Yb.float()).all() and Yb.float().abs().max() > 0
    assert torch.equal(ys[0].view(torch.int16), Yb.view(torch.int16)), (M, N, K, kind)
    assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16))
    assert n1 - n0 == (0 if mode == NATIVE else 2), (n0, n1)
    return ys[0]


@pytest.mark.parametrize("N,K", [(48, 192), (128, 1536)])
@pytest.mark.parametrize("M", [17, 33, 40, 64])
def test_gemv_rows(M, N, K):
    """k_gemv MREP 2, 3, 4: few tiles, 4 waves.  K = 192 is 6 chunks over 4 waves:
    ranges start on odd chunks and cut chunk pairs (half-loads)."""
    run(M, N, K, "gemv")


def test_gemv_split_k_handoff():
    run(40, 1024, 4096, "gemv", ksplit=4)


@pytest.mark.parametrize("N,K", [(4608, 1536), (8192, 192), (16384, 64)])
@pytest.mark.parametrize("M", [24, 64])
def test_gemvw_rows(M, N, K):
    """288 / 512 / 1,024 tiles: 1, 2 and 4 tiles per workgroup; K = 64 is a single chunk pair."""
    run(M, N, K, "gemvw")


# N = 96: the smallest k_gemm<32> width (above 64 rows N % 32 != 0, e.g. N = 48, is
# rejected by the launcher for bf16 and FP8 operands alike)
@pytest.mark.parametrize("N,K,kind", [(96, 192, "gemm32"), (4608, 192, "gemm64")])
@pytest.mark.parametrize("M", [65, 200])
def test_gemm_rows(M, N, K, kind):
    run(M, N, K, kind)


def test_gemm_norm_rows_above_256():
    run(300, 4608, 1536, "gemm64", xf=1)


FORMS = dict(bias=dict(bias=True), res=dict(epi="res", res=True), silu_mul=dict(epi="silu_mul"), norm=dict(xf=1),
             norm_w=dict(xf=1, norm_w=True))


@pytest.mark.parametrize("M,kind", [(40, "gemv"), (200, "gemm32")])
@pytest.mark.parametrize("case", sorted(FORMS))
def test_forms(M, kind, case):
    run(M, 48 if M == 40 else 96, 192, kind, **FORMS[case])


@pytest.mark.parametrize("M,kind", [(40, "gemv"), (200, "gemm32")])
def test_form_norm_bias(M, kind):
    """RMSNorm on load + norm weight + bias (vv_gemm_bf16_norm takes no bias: the
    reference is the dequantise fallback, itself bit-equal to bf16 by the tests above)."""
    N = 48 if M == 40 else 96
    Y = run(M, N, 192, kind, xf=1, norm_w=True)
    L = _lib.lib()
    _, codes, e = _weight(N, 192)
    g = torch.Generator(device=dev).manual_seed(M)
    A = torch.randn(M, 192, device=dev, generator=g).bfloat16()
    b = (0.1 * torch.randn(N, device=dev, generator=g)).bfloat16()
    nw = (1.0 + 0.1 * torch.randn(192, device=dev, generator=g)).bfloat16()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ys = []
    n0 = launches()
    for on in (1, 1, 0):
        L.vv_gemv_w8(on)
        Yq = torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
        _lib.check(L.vv_gemm_w8(M, N, 192, P(A), 192, P(codes), P(e), 1, P(nw), 1e-6, P(b), 0, P(Yq), N, None, None, st),
                   "gemm_w8")
        ys.append(Yq)
    L.vv_gemv_w8(1)
    torch.cuda.synchronize()
    assert launches() - n0 == 1
    assert torch.isfinite(ys[2].float()).all()
    assert torch.equal(ys[0].view(torch.int16), ys[2].view(torch.int16))
    assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16))


def test_every_code_and_the_exponent_range():
    """All 254 finite e4m3 codes in every row, one exponent per row over the
    format's range [-100, 100]: the in-register conversion is the dequantise
    pass's, value for value (an identity A reads the weights out)."""
    N, K, M = 208, 256, 64
    codes = torch.arange(256, device=dev, dtype=torch.uint8)
    codes = torch.where((codes & 0x7f) == 0x7f, torch.zeros_like(codes), codes)      # NaN codes never occur
    codes = codes[None, :].repeat(N, 1).view(torch.float8_e4m3fn)
    e = (torch.arange(N, device=dev) - 100).clamp(-100, 100).to(torch.int8)
    Wd = dequantize_rows(codes, e)
    Wp, c8 = mfma_pack(Wd).contiguous(), mfma_pack8(codes).contiguous()
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n0 = launches()
    for k0 in range(0, K, M):
        A = torch.zeros(M, K, device=dev, dtype=torch.bfloat16)
        A[torch.arange(M), k0 + torch.arange(M)] = 1
        Y8 = torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
        Yb = torch.full_like(Y8, float("nan"))
        _lib.check(L.vv_gemm_w8(M, N, K, P(A), K, P(c8), P(e), 0, None, 0.0, None, 0, P(Y8), N, None, None, st), "w8")
        _lib.check(L.vv_gemm_bf16(M, N, K, P(A), K, P(Wp), None, 0, P(Yb), N, None, None, None, st), "bf16")
        torch.cuda.synchronize()
        assert torch.equal(Yb, Wd[:, k0:k0 + M].t())                               # the read-out is exact
        assert torch.equal(Y8.view(torch.int16), Yb.view(torch.int16)), k0
    assert launches() == n0


def test_switch_forces_the_dequantise_pass():
    """vv_gemv_w8(0): the same M = 40 call dequantises once and gives the same bits."""
    Y = run(40, 48, 192, "gemv")
    L = _lib.lib()
    L.vv_gemv_w8(0)
    try:
        n0 = launches()
        Y0 = run(40, 48, 192, "gemv", mode=2)
        assert launches() - n0 == 2                                                 # run() calls twice
    finally:
        L.vv_gemv_w8(1)
    assert torch.equal(Y.view(torch.int16), Y0.view(torch.int16))
    n0 = launches()
    run(40, 48, 192, "gemv")
    assert launches() == n0


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


def test_engine_passes_run_no_dequantise():
    """max_batch 12: a 40-row prompt pass and a 24-row decode pass (12 dialogues x
    [cond | uncond]), FP8 engine vs bf16 engine on the fake-quantised weights:
    bit-equal, and the dequantise counter stands still.  (Before the W8
    instantiations it rose by one per quantised matrix per pass.)"""
    cfg = tiny_config()
    q, b = _pair(cfg, seed=31, max_batch=12)
    H = cfg.decoder_config.hidden_size
    g = torch.Generator().manual_seed(2)
    n0 = launches()
    x = torch.randn(40, H, generator=g).bfloat16().to(dev)
    slots, pos = torch.zeros(40, **I32), torch.arange(40, **I32)
    out_idx = torch.tensor([39], **I32)
    hq, lq = q.lm_forward(x, slots, pos, out_idx)
    hb, lb = b.lm_forward(x, slots, pos, out_idx)
    torch.cuda.synchronize()
    assert torch.isfinite(hq.float()).all()
    assert torch.equal(hq.view(torch.int16), hb.view(torch.int16)) and torch.equal(lq, lb)
    xs = torch.randn(24, H, generator=g).bfloat16().to(dev)
    slots = torch.arange(24, **I32)
    pos = torch.where(slots == 0, 40, 0).to(torch.int32)
    args = (xs, slots, pos, torch.arange(24, **I32))
    hq, lq = q.lm_forward(*args)
    hb, lb = b.lm_forward(*args)
    torch.cuda.synchronize()
    assert torch.isfinite(hq.float()).all()
    assert torch.equal(hq.view(torch.int16), hb.view(torch.int16)) and torch.equal(lq, lb)
    assert launches() == n0
    q.close()
    b.close()


@pytest.fixture(scope="module")
def tiny_fp8_b9():
    cfg = tiny_config()
    sd = _sd(cfg, 33)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, dev, max_batch=9, max_ctx=256, weight_dtype=FP8)
    m.set_ddpm_inference_steps(5)
    yield cfg, sd, m
    m.engine.close()


# 6 steps; the first 4 run all 9 dialogues
SCHED9 = [[D, D, D, D, D, X], [D, E, S, D, D, X], [S, D, D, D, D, X], [D, D, E, S, D, X], [D, D, D, X],
          [D, E, S, D, X], [S, D, D, X], [D, D, D, D, X], [S, D, E, S, D, X]]


def test_decode_b9_vs_oracle_on_fake_quantised(tiny_fp8_b9):
    """18 LM rows per decode step (9 dialogues x [cond | uncond]): every quantised
    projection runs k_gemv<2>'s W8 instantiation.  DESIGN.md §4's per-step bounds."""
    cfg, sd, m = tiny_fp8_b9
    L = _lib.lib()
    assert L.vv_weights_quantized(m.engine.h) == 1
    assert L.vv_lm_ffn_active(m.engine.h, 18) == 0 and L.vv_lm_attn_active(m.engine.h, 18, 64) == 0
    inp = synthetic_inputs(batch=9, speakers=1, voice_seconds=0, text_tokens=8, seed=39, hop=cfg.hop)
    fsd = fake_quantize_state_dict(sd, cfg)
    rec, seqs, _, _ = oracle_run(fsd, cfg, inp, SCHED9, IDS, 5, None, 1234)
    n0 = launches()
    got, sess = teacher_forced(m, inp, SCHED9, rec, TK, 1234)
    assert torch.equal(sess.result().sequences, seqs)
    per_step_check(got, rec, None, "tiny FP8 B=9")
    print("dequantise passes during the B = 9 run (prompt rows <= 16 per pass may take k_gemv1's fallback):",
          launches() - n0)


def test_graph_replay_matches_eager_b9(tiny_fp8_b9):
    cfg, sd, m = tiny_fp8_b9
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 151000, (9, 12), generator=g)
    mask = torch.ones(9, 12, dtype=torch.long)
    outs = []
    for graphs in (False, True):
        torch.manual_seed(77)
        outs.append(m.generate(input_ids=ids, attention_mask=mask, tokenizer=TK, cfg_scale=1.3, forced_tokens=SCHED9,
                               use_graphs=graphs, show_progress_bar=False))
    assert len(m._graph_cache) >= 1
    assert torch.equal(outs[0].sequences, outs[1].sequences)
    for b in range(9):
        a0, a1 = outs[0].speech_outputs[b], outs[1].speech_outputs[b]
        if a0 is None and a1 is None:
            continue
        a0, a1 = a0.cpu(), a1.cpu()
        assert torch.isfinite(a0.float()).all() and torch.equal(a0, a1)
