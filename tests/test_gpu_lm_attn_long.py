"""The one-launch LM attention kernel past 4,096 keys (lm_attn.hip: k_lm_attn's long
form, the per-engine option lm_attn_max_keys / vv_set_lm_attn_max_keys, default 4,096).

A pass planned past 4,096 keys runs the long instantiation: an attention unit covers
32 s keys, s = ceil(len / 4,096) per row inside the kernel, its wave carrying (m, l, O)
over the s steps.  Rows of at most 4,096 keys have s = 1 and must give the short form's
bits; longer rows are held to the oracle and to the three launches within the bounds
test_gpu_lm.py uses for that comparison (rel L2 < 2e-2, cosine > 0.999).  Random keys
give near-uniform attention at 16K keys, where one lost unit hides inside 2e-2, so a last
test plants one dominant key per case at the unit and step edges.

Engines have the 1.5B layer shapes (H 1536, 12 / 2 heads of 128, I 8960) and are built one
after another: a one-launch kernel runs only while its context is the device's only
registered one.  Long contexts are filled with vv_diag_kv_write, not a prefill.
"""
import ctypes
import gc

import pytest
import torch
import torch.nn.functional as F

from gpu_util import cos, rel_err
from oracle import lm as olm
from sync_counters import assert_counters_consistent
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.weights import fake_quantize_state_dict, synthetic_state_dict

pytestmark = pytest.mark.gpu
dev = "cuda"
I32 = dict(dtype=torch.int32, device=dev)
BF = dict(dtype=torch.bfloat16, device=dev)
VALID = [151643, 151652, 151653, 151654]
FP8 = "fp8_e4m3"
H, I, NH, NKV, HD = 1536, 8960, 12, 2, 128
LMP = "model.language_model."


@pytest.fixture(autouse=True)
def _switches():
    gc.collect()
    yield
    _lib.lib().vv_lm_attn(1)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _cfg(layers=2):
    return tiny_config(hidden=H, layers=layers, heads=NH, kv_heads=NKV, inter=I)


def _sd(cfg, seed):
    return synthetic_state_dict(cfg, seed=seed, device="cpu", mode="test", with_acoustic_encoder=False)


def _engine(cfg, sd, max_batch, max_ctx, **kw):
    return Engine(cfg, sd, dev, max_batch=max_batch, max_ctx=max_ctx, valid_ids=VALID, **kw)


def _close(eng):
    eng.close()
    del eng
    gc.collect()


def kv_read(eng, layers, slot, p0, p1):
    k = torch.empty(layers, NKV, p1 - p0, HD, **BF)
    v = torch.empty_like(k)
    _lib.check(_lib.lib().vv_diag_kv_read(eng.h, slot, p0, p1, P(k), P(v)), "diag_kv_read")
    torch.cuda.synchronize()
    return k, v


def kv_write(eng, slot, p0, p1, k, v):
    k, v = k.to(dev).contiguous(), v.to(dev).contiguous()
    _lib.check(_lib.lib().vv_diag_kv_write(eng.h, slot, p0, p1, P(k), P(v)), "diag_kv_write")
    torch.cuda.synchronize()


def oracle_sd(sd):
    return {k[len(LMP):]: v for k, v in sd.items() if k.startswith(LMP)}


# ------------------------------------------------------------------ 1. which path runs
def test_active_and_errors():
    L = _lib.lib()
    cfg = _cfg()
    sd = _sd(cfg, 91)
    a = _engine(cfg, sd, 16, 16384, lm_attn_max_keys=16384)
    assert L.vv_lm_attn_max_keys(a.h) == 16384 and a.lm_attn_max_keys == 16384
    assert L.vv_lm_attn_active(a.h, 2, 4097) == 1 and L.vv_lm_attn_active(a.h, 16, 16384) == 1
    assert L.vv_lm_attn_active(a.h, 2, 64) == 1 and L.vv_lm_attn_active(a.h, 17, 16384) == 0
    assert L.vv_set_lm_attn_max_keys(a.h, 8192) != 0 and b"vv_set_lm_attn_max_keys after vv_finalize" in L.vv_last_error()
    assert L.vv_lm_attn_max_keys(a.h) == 16384
    _close(a)
    b = _engine(cfg, sd, 2, 16384)
    assert L.vv_lm_attn_max_keys(b.h) == 4096 and b.lm_attn_max_keys is None
    assert L.vv_lm_attn_active(b.h, 2, 4096) == 1 and L.vv_lm_attn_active(b.h, 2, 4097) == 0
    _close(b)
    # the long form reads a bf16 cache: an FP8-KV engine keeps the short form and, past 4,096 keys, today's launches
    f = _engine(cfg, sd, 2, 8192, lm_attn_max_keys=8192, kv_dtype=FP8, lm_attn_kv8=True)
    assert L.vv_lm_attn_max_keys(f.h) == 8192
    assert L.vv_lm_attn_active(f.h, 2, 4096) == 1 and L.vv_lm_attn_active(f.h, 2, 4097) == 0
    _close(f)
    with pytest.raises(ValueError, match="outside"):
        _engine(cfg, sd, 2, 8192, lm_attn_max_keys=8193)
    with pytest.raises(ValueError, match="outside"):
        _engine(cfg, sd, 2, 8192, lm_attn_max_keys=4095)
    with pytest.raises(ValueError, match="tensor parallelism"):
        Engine(cfg, sd, dev, max_batch=2, max_ctx=8192, tp_size=2, lm_attn_max_keys=8192)
    with pytest.raises(ValueError, match="outside"):
        VibeVoiceForConditionalGenerationInference(cfg, sd, dev, max_ctx=8192, lm_attn_max_keys=9000)


# ------------------------------------------------------------------ 2. bits at 4,096 keys or fewer
SHORT_LENS = (1, 31, 32, 33, 64, 200, 4093)


def _short_run(eng, rows, xs, plan_max_pos):
    """Fill the slots, two decode steps; hidden bits, logits, the appended rows, and step 2 again."""
    L = _lib.lib()
    R = len(SHORT_LENS)
    for r, (k, v) in enumerate(rows):
        kv_write(eng, r, 0, k.shape[2], k, v)
    ar = torch.arange(R).to(**I32)
    out = []
    for s in (0, 1, 1):
        mp = plan_max_pos if plan_max_pos is not None else max(SHORT_LENS) + s
        assert L.vv_lm_attn_active(eng.h, R, mp + 1) == 1
        h, lg = eng.lm_forward(xs[s], ar, (torch.tensor(SHORT_LENS) + s).to(**I32), ar, max_pos=mp)
        torch.cuda.synchronize()
        out.append((bits(h), lg.cpu()))
    kv = [tuple(bits(t) for t in kv_read(eng, 2, r, n, n + 2)) for r, n in enumerate(SHORT_LENS)]
    eng.check_sync()
    assert_counters_consistent(eng)
    return out, kv


def test_short_rows_compute_the_short_forms_bits():
    """Engine A: max_ctx 4,096, default options (the short form).  Engine B: max_ctx 8,192 with the
    option, planned at max_ctx - 1 as generate() plans it (the long form).  Same weights, same cache."""
    cfg = _cfg()
    sd = _sd(cfg, 92)
    g = torch.Generator().manual_seed(93)
    rows = [(torch.randn(2, NKV, n, HD, generator=g).bfloat16(), torch.randn(2, NKV, n, HD, generator=g).bfloat16())
            for n in SHORT_LENS]
    xs = [torch.randn(len(SHORT_LENS), H, generator=g).bfloat16().to(dev) for _ in range(2)]
    a = _engine(cfg, sd, 4, 4096)
    ra, ka = _short_run(a, rows, xs, None)
    _close(a)
    b = _engine(cfg, sd, 4, 8192, lm_attn_max_keys=8192)
    rb, kb = _short_run(b, rows, xs, 8191)
    _close(b)
    for s, ((h, lg), (hb, lgb)) in enumerate(zip(ra, rb)):
        print(f"step {s}: {(h != hb).sum().item()} of {h.numel()} hidden values differ")
        assert torch.isfinite(lg).all() and torch.equal(h, hb) and torch.equal(lg, lgb)
    for run in (ra, rb):   # repeat runs
        assert torch.equal(run[1][0], run[2][0]) and torch.equal(run[1][1], run[2][1])
    for (k, v), (k2, v2) in zip(ka, kb):
        assert k.any() and v.any() and torch.equal(k, k2) and torch.equal(v, v2)


# ------------------------------------------------------------------ 2b. FP8 weights, long form
W8_KEYS = (4093, 4097, 8189)   # keys of each row at step 1: s = 1; s = 2 with a one-key tail unit; s = 2 ending mid-unit


def _w8_long_run(eng, rows, xs):
    """Fill the slots through kv_write, two decode steps planned at 8,192 keys; hidden bits, logits, the appended rows."""
    L = _lib.lib()
    R = len(W8_KEYS)
    for r, (k, v) in enumerate(rows):
        kv_write(eng, r, 0, k.shape[2], k, v)
    ar = torch.arange(R).to(**I32)
    out = []
    for s in range(2):
        assert L.vv_lm_attn_active(eng.h, R, 8192) == 1
        h, lg = eng.lm_forward(xs[s], ar, (torch.tensor(W8_KEYS) - 1 + s).to(**I32), ar, max_pos=8191)
        torch.cuda.synchronize()
        out.append((bits(h), lg.cpu()))
    kv = [tuple(bits(t) for t in kv_read(eng, 2, r, n - 1, n + 1)) for r, n in enumerate(W8_KEYS)]
    eng.check_sync()
    assert_counters_consistent(eng)
    return out, kv


def test_w8_long_form_bit_identical_to_bf16_on_dequantised():
    """k_lm_attn<W8, 0, LONG>: an FP8 engine with lm_attn_w8 and lm_attn_max_keys = 8,192 against a bf16 engine
    on the dequantised matrices with the same context options (test_gpu_w8_lm_attn.py's bit test, past 4,096 keys)."""
    cfg = _cfg()
    sd = _sd(cfg, 191)
    g = torch.Generator().manual_seed(192)
    rows = [(torch.randn(2, NKV, n - 1, HD, generator=g).bfloat16(), torch.randn(2, NKV, n - 1, HD, generator=g).bfloat16())
            for n in W8_KEYS]
    xs = [torch.randn(len(W8_KEYS), H, generator=g).bfloat16().to(dev) for _ in range(2)]
    q = _engine(cfg, sd, 2, 8192, lm_attn_max_keys=8192, weight_dtype=FP8, lm_attn_w8=True)
    assert q.weights_quantized() and _lib.lib().vv_lm_attn_w8(q.h) == 1
    rq, kq = _w8_long_run(q, rows, xs)
    _close(q)
    b = _engine(cfg, fake_quantize_state_dict(sd, cfg), 2, 8192, lm_attn_max_keys=8192)
    assert not b.weights_quantized()
    rb, kb = _w8_long_run(b, rows, xs)
    _close(b)
    for s, ((h, lg), (hb, lgb)) in enumerate(zip(rq, rb)):
        print(f"step {s}: {(h != hb).sum().item()} of {h.numel()} hidden values differ")
        assert torch.isfinite(lg).all() and torch.isfinite(h.view(torch.bfloat16).float()).all()
        assert torch.equal(h, hb) and torch.equal(lg, lgb)
    for (k, v), (k2, v2) in zip(kq, kb):
        assert k.any() and v.any() and torch.equal(k, k2) and torch.equal(v, v2)


# ------------------------------------------------------------------ 3. past 4,096 keys
LONG_LENS = (4095, 4096, 4097, 8191, 8192, 8193, 12289, 16381, 33, 1)


def test_long_rows_vs_oracle_and_three_launches():
    L = _lib.lib()
    cfg = _cfg()
    sd = _sd(cfg, 94)
    lcfg, osd = dict(cfg.decoder_config), oracle_sd(sd)
    R = 16
    lens = [LONG_LENS[r % len(LONG_LENS)] for r in range(R)]
    eng = _engine(cfg, sd, 8, 16384, lm_attn_max_keys=16384)
    g = torch.Generator(device=dev).manual_seed(95)
    kvs = []
    for r, n in enumerate(lens):
        k = torch.randn(2, NKV, n, HD, generator=g, **BF)
        v = torch.randn(2, NKV, n, HD, generator=g, **BF)
        kv_write(eng, r, 0, n, k, v)
        kr, vr = kv_read(eng, 2, r, 0, n)
        kv = olm.RowKV(2)
        kv.k, kv.v = [kr[l].cpu() for l in range(2)], [vr[l].cpu() for l in range(2)]
        kvs.append(kv)
    ar = torch.arange(R).to(**I32)
    gc_ = torch.Generator().manual_seed(96)
    for s in range(3):
        x = torch.randn(R, H, generator=gc_).bfloat16()
        pos = (torch.tensor(lens) + s).to(**I32)
        ref = olm.forward_rows(osd, lcfg, x[:, None], kvs)[:, -1]
        assert L.vv_lm_attn_active(eng.h, R, 16384) == 1
        h1, lg1 = eng.lm_forward(x.to(dev), ar, pos, ar, max_pos=16383)
        torch.cuda.synchronize()
        h1, lg1 = h1.clone(), lg1.clone()
        h2, lg2 = eng.lm_forward(x.to(dev), ar, pos, ar, max_pos=16383)
        torch.cuda.synchronize()
        assert torch.equal(bits(h1), bits(h2)) and torch.equal(lg1, lg2)
        L.vv_lm_attn(0)
        assert L.vv_lm_attn_active(eng.h, R, 16384) == 0
        h0, _ = eng.lm_forward(x.to(dev), ar, pos, ar, max_pos=16383)
        torch.cuda.synchronize()
        L.vv_lm_attn(1)
        for r in range(R):
            e_o, c_o = rel_err(h1[r], ref[r]), cos(h1[r], ref[r])
            e_3, c_3 = rel_err(h1[r], h0[r]), cos(h1[r], h0[r])
            print(f"step {s} row {r} len {lens[r] + s}: oracle rel {e_o:.2e} cos {c_o:.5f}; three launches rel {e_3:.2e} cos {c_3:.5f}")
            assert e_o < 2e-2 and c_o > 0.999 and e_3 < 2e-2 and c_3 > 0.999, (s, r)
    eng.check_sync()
    assert_counters_consistent(eng)
    _close(eng)


# ------------------------------------------------------------------ 4. no unit or step may be droppable
PLANT_LEN = 16381                      # s = 4: units of 128 keys, steps of 32
PLANT_AT = (0, 127, 31, 32, 128, PLANT_LEN - 1)   # unit 0's first / last key, a step edge, a unit edge, the last cached key


def _query(osd, lcfg, x, pos):
    """Layer 0's RoPE'd query rows [NH][HD] of the token x at `pos` (the oracle's statement)."""
    a = olm.rms(x[None, None], osd["layers.0.input_layernorm.weight"], lcfg["rms_norm_eps"])
    q = F.linear(a, osd["layers.0.self_attn.q_proj.weight"], osd["layers.0.self_attn.q_proj.bias"])[0, 0].view(NH, HD)
    c, s = olm.rope_cos_sin(torch.tensor([pos]), HD, lcfg["rope_theta"], x.dtype)
    return q * c + olm._rot(q) * s


def test_planted_key_at_unit_and_step_edges():
    L = _lib.lib()
    cfg = _cfg(layers=1)
    sd = _sd(cfg, 97)
    lcfg, osd = dict(cfg.decoder_config), oracle_sd(sd)
    g = torch.Generator().manual_seed(98)
    n = PLANT_LEN
    base_k = (0.25 * torch.randn(1, NKV, n, HD, generator=g)).bfloat16()
    base_v = (0.25 * torch.randn(1, NKV, n, HD, generator=g)).bfloat16()
    x = torch.randn(H, generator=g).bfloat16()
    q_ref = _query(osd, lcfg, x, n).float()
    eng = _engine(cfg, sd, 1, 16384, lm_attn_max_keys=16384)
    kv_write(eng, 0, 0, n, base_k, base_v)
    one, zero = torch.tensor([0]).to(**I32), torch.tensor([0]).to(**I32)
    # the row's RoPE'd query as the kernel's phase 1 wrote it (vv_diag_lm_qkv after a pass); the oracle's agrees
    eng.lm_forward(x[None].to(dev), zero, torch.tensor([n]).to(**I32), one, max_pos=16383)
    qd, kd, vd = torch.empty(1, NH * HD, **BF), torch.empty(1, NKV, HD, **BF), torch.empty(1, NKV, HD, **BF)
    arr = lambda *v: (ctypes.c_int * len(v))(*v)
    _lib.check(L.vv_diag_lm_qkv(eng.h, 1, 0, arr(0), arr(n), P(qd), P(kd), P(vd)), "diag_lm_qkv")
    q = qd.view(NH, HD).float().cpu()
    assert rel_err(q, q_ref) < 2e-2 and cos(q, q_ref) > 0.999
    # K aligned to the first query head of each kv head: a score of 40 against O(1) for the rest
    pk = torch.stack([q[kh * (NH // NKV)] * (40.0 * HD ** 0.5 / q[kh * (NH // NKV)].pow(2).sum()) for kh in range(NKV)]).bfloat16()
    pv = (24.0 * torch.sign(torch.randn(NKV, HD, generator=g))).bfloat16()

    def oracle(k, v):
        kv = olm.RowKV(1)
        kv.k, kv.v = [k[0]], [v[0]]
        return olm.forward_rows(osd, lcfg, x[None, None], [kv], commit=False)[0, -1]

    for at in PLANT_AT:
        k, v = base_k.clone(), base_v.clone()
        k[0, :, at], v[0, :, at] = pk, pv
        full = oracle(k, v)
        k0, v0 = k.clone(), v.clone()
        k0[0, :, at], v0[0, :, at] = 0, 0
        gone = oracle(k0, v0)
        d = rel_err(gone, full)
        print(f"key {at}: the oracle without it differs by rel {d:.3f}")
        assert d >= 10 * 2e-2, (at, d)
        kv_write(eng, 0, at, at + 1, k[:, :, at:at + 1], v[:, :, at:at + 1])
        assert L.vv_lm_attn_active(eng.h, 1, 16384) == 1
        h, _ = eng.lm_forward(x[None].to(dev), zero, torch.tensor([n]).to(**I32), one, max_pos=16383)
        torch.cuda.synchronize()
        e, c = rel_err(h[0], full), cos(h[0], full)
        print(f"key {at}: one launch vs oracle rel {e:.2e} cos {c:.5f}")
        assert e < 2e-2 and c > 0.999, at
        kv_write(eng, 0, at, at + 1, base_k[:, :, at:at + 1], base_v[:, :, at:at + 1])
    eng.check_sync()
    assert_counters_consistent(eng)
    _close(eng)


# ------------------------------------------------------------------ 6. generate() end to end
def test_generate_default_max_ctx_equals_an_engine_sized_to_its_run():
    """The constructor's default max_ctx = 8,192 plans every captured decode graph at 8,191 keys: with the
    option those graphs hold the long form, and a graph-replayed generate() must give the tokens and audio of
    a max_ctx = 4,096 model with default options (the short form) on the same weights."""
    from vibevoice_amd.synthetic import tokenizer_ids
    L = _lib.lib()
    TK = tokenizer_ids()
    D, E, S, X = TK.speech_diffusion_id, TK.speech_end_id, TK.speech_start_id, TK.eos_token_id
    cfg = _cfg()
    cfg.decoder_config["max_position_embeddings"] = 8192   # (the constructor clamps max_ctx to it; 1.5B's is 65,536)
    sd = _sd(cfg, 99)
    M = VibeVoiceForConditionalGenerationInference
    ids = torch.randint(0, 151000, (1, 12), generator=torch.Generator().manual_seed(3))
    mask = torch.ones(1, 12, dtype=torch.long)
    sched = [[D, D, D, E, S, D, X]]
    outs = []
    for kw in (dict(lm_attn_max_keys=8192), dict(max_ctx=4096)):
        m = M(cfg, sd, dev, max_batch=1, **kw)
        eng = m.engine
        if "max_ctx" not in kw:
            assert eng.max_ctx == 8192 and m.lm_attn_max_keys == 8192 and L.vv_lm_attn_max_keys(eng.h) == 8192
        assert L.vv_lm_attn_active(eng.h, 2, eng.max_ctx) == 1
        m.set_ddpm_inference_steps(5)
        torch.manual_seed(77)
        o = m.generate(input_ids=ids, attention_mask=mask, tokenizer=TK, cfg_scale=1.3, forced_tokens=sched,
                       use_graphs=True, show_progress_bar=False)
        assert len(m._graph_cache) >= 1
        outs.append((o.sequences.clone().cpu(), o.speech_outputs[0].clone().cpu()))
        eng.check_sync()
        assert_counters_consistent(eng)
        eng.close()
        del m, eng
        gc.collect()
    (seq, audio), (seq0, audio0) = outs
    assert torch.isfinite(audio.float()).all() and audio.float().abs().max() > 0
    assert torch.equal(seq, seq0) and torch.equal(bits(audio), bits(audio0))
