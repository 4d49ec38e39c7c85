"""The one-launch LM attention kernel on an FP8 KV cache (lm_attn.hip: k_lm_attn's
KVQ forms, the per-engine option lm_attn_kv8 / vv_set_lm_attn_kv8, default off).

KVQ = 1 stages the pass's K / V rows, runs the rows a unit needs through the cache's
e4m3 row quantiser inside the launch, stores codes + exponents and reads codes.
Nothing else in the tree computes those bits, so the kernel has a diagnostic twin,
KVQ = 2 (vv_lm_attn_kvround on a bf16 engine): the same data flow and quantiser,
the rows stored dequantised in a bf16 cache and read as bf16.  A power-of-two row
scale commutes with the MFMAs' fp32 sums (test_gpu_kv8.py asserts that identity for
k_attn over row magnitudes 2^-6 .. 2^6; the rows here stay inside it), so engine A
(FP8 KV, the option) must equal engine B (bf16 KV under the round trip) bit for
bit once B's cache holds A's dequantised rows.  The quantiser itself is pinned to
the CPU statement (weights.fake_quantize_kv) through a plain bf16 engine's layer-0
rows, and the whole path to the three launches and to the reference on
fake-quantised K / V (tests/kv8_ref.py) within the project's bounds for the one
launch against the three: rel L2 < 2e-2, cosine > 0.999.

All engines are the smallest the kernel accepts (H 1536, 12 / 2 heads of 128, I
8960, 2 layers), built one after another: a one-launch kernel runs only while its
context is the device's only registered one.
"""
import ctypes
import gc

import pytest
import torch

import kv8_ref
from gpu_util import cos, rel_err
from oracle import lm as olm
from sync_counters import assert_counters_consistent
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.synthetic import tokenizer_ids
from vibevoice_amd.weights import (fake_quantize_kv, fake_quantize_state_dict, synthetic_state_dict,
                                   write_synthetic_checkpoint)

pytestmark = pytest.mark.gpu
dev = "cuda"
I32 = dict(dtype=torch.int32, device=dev)
BF = dict(dtype=torch.bfloat16, device=dev)
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
    _lib.lib().vv_lm_attn_kvround(0)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _cfg():
    return tiny_config(hidden=H, layers=2, heads=NH, kv_heads=NKV, inter=I)


def _sd(cfg, seed):
    return synthetic_state_dict(cfg, seed=seed, device="cpu", mode="test", with_acoustic_encoder=False)


def _engine(cfg, sd, max_batch, weight_dtype=None, kv_dtype=None, **kw):
    return Engine(cfg, sd, dev, max_batch=max_batch, max_ctx=MAX_CTX, valid_ids=VALID, weight_dtype=weight_dtype,
                  kv_dtype=kv_dtype, **kw)


def _close(eng):
    eng.close()
    del eng
    gc.collect()


def kv_read(eng, slot, p0, p1):
    k = torch.empty(2, NKV, p1 - p0, HD, **BF)
    v = torch.empty_like(k)
    _lib.check(_lib.lib().vv_diag_kv_read(eng.h, slot, p0, p1, P(k), P(v)), "diag_kv_read")
    torch.cuda.synchronize()
    return k, v


def kv_write(eng, slot, p0, p1, k, v):
    k, v = k.to(dev).contiguous(), v.to(dev).contiguous()
    _lib.check(_lib.lib().vv_diag_kv_write(eng.h, slot, p0, p1, P(k), P(v)), "diag_kv_write")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. which path runs
def test_active():
    cfg = _cfg()
    sd = _sd(cfg, 81)
    L = _lib.lib()
    rows = (1, 2, 3, 16, 17)
    act = lambda e, keys=64: [L.vv_lm_attn_active(e.h, r, keys) for r in rows]   # noqa: E731
    a = _engine(cfg, sd, 8, kv_dtype=FP8, lm_attn_kv8=True)
    assert L.vv_kv_dtype(a.h) == 1 and L.vv_lm_attn_kv8(a.h) == 1
    assert act(a) == [1, 1, 1, 1, 0]                       # (0 on the code as it stood before the option)
    L.vv_lm_attn(0)
    assert act(a) == [0, 0, 0, 0, 0]
    L.vv_lm_attn(1)
    assert act(a) == [1, 1, 1, 1, 0]
    assert L.vv_set_lm_attn_kv8(a.h, 0) != 0 and b"vv_set_lm_attn_kv8 after vv_finalize" in L.vv_last_error()
    assert L.vv_lm_attn_kv8(a.h) == 1
    _close(a)
    big = Engine(cfg, sd, dev, max_batch=1, max_ctx=4608, valid_ids=VALID, kv_dtype=FP8, lm_attn_kv8=True)
    assert [L.vv_lm_attn_active(big.h, 2, k) for k in (4096, 4097)] == [1, 0]
    _close(big)
    off = _engine(cfg, sd, 8, kv_dtype=FP8)                # FP8 KV without the option: the three launches
    assert L.vv_lm_attn_kv8(off.h) == 0 and act(off) == [0, 0, 0, 0, 0]
    L.vv_lm_attn_kvround(1)                                # (the diagnostic is a bf16-KV engine's)
    assert act(off) == [0, 0, 0, 0, 0]
    L.vv_lm_attn_kvround(0)
    _close(off)
    # FP8 weights + FP8 KV: both options, or the three launches (lm_attn_w8 alone is refused in Python)
    with pytest.raises(ValueError, match="kv_dtype"):
        _engine(cfg, sd, 8, weight_dtype=FP8, kv_dtype=FP8, lm_attn_w8=True)
    for w8, kv8, want in ((False, False, 0), (False, True, 0), (True, True, 1)):
        q = _engine(cfg, sd, 8, weight_dtype=FP8, kv_dtype=FP8, lm_attn_w8=w8, lm_attn_kv8=kv8)
        assert q.weights_quantized() and L.vv_kv_dtype(q.h) == 1
        assert act(q) == [want] * 4 + [0], (w8, kv8)
        _close(q)
    b = _engine(cfg, sd, 8)                                # a bf16 engine: as before
    assert L.vv_lm_attn_kv8(b.h) == 0 and act(b) == [1, 1, 1, 1, 0]
    L.vv_lm_attn(0)
    assert act(b) == [0, 0, 0, 0, 0]
    L.vv_lm_attn(1)
    L.vv_lm_attn_kvround(1)
    assert act(b) == [1, 1, 1, 1, 0]
    L.vv_lm_attn_kvround(0)
    _close(b)


# ------------------------------------------------------------------ 2, 4. bit identity; the quantiser
ROWS = (1, 2, 3, 6, 16)
LENS = (1, 31, 32, 33, 64, 200)     # per-row context lengths, cycled: both sides of the 32-key unit edge, a single key
K_EXP = ((-3, 1), (2, -1))          # [layer][kv head]: k_proj rows (and bias) times 2^e
V_EXP = ((-5, 2), (5, -2))          # ... v_proj: the appended rows' exponents cover several binades, inside 2^-6 .. 2^6


def _spread_exponents(cfg, sd):
    """Every k_proj / v_proj output row of (layer, kv head) and its bias times a power of
    two: the cached rows of that head scale exactly (RoPE is linear), so rows of different
    heads, layers and of K and V land in different binades."""
    for l in range(cfg.decoder_config.num_hidden_layers):
        p = f"{LMP}layers.{l}.self_attn."
        for n, ex in (("k", K_EXP[l]), ("v", V_EXP[l])):
            e = torch.tensor(ex, dtype=torch.int32).repeat_interleave(HD)
            for t in ("weight", "bias"):
                w = sd[p + n + "_proj." + t]
                sd[p + n + "_proj." + t] = torch.ldexp(w.float(), e[:, None] if w.dim() == 2 else e).to(w.dtype)
    return sd


def _lens(R):
    return [LENS[r % len(LENS)] for r in range(R)]


def _steps(eng, xs, R, extra):
    """2 decode steps on the R rows; (hidden bits, logits) per step, the rows both steps
    appended (both layers), and with `extra` step 2 again as it is and under vv_lm_attn(15)."""
    L = _lib.lib()
    lens = _lens(R)
    ar = torch.arange(R).to(**I32)

    def step(s):
        assert L.vv_lm_attn_active(eng.h, R, max(lens) + s + 1) == 1, (R, s)
        h, lg = eng.lm_forward(xs["step"][s], ar, (torch.tensor(lens) + s).to(**I32), ar)
        torch.cuda.synchronize()
        return bits(h), lg.cpu()

    def appended():
        return [tuple(bits(t) for t in kv_read(eng, r, n, n + 2)) for r, n in enumerate(lens)]

    out = {"steps": [step(0), step(1)]}
    out["kv"] = appended()
    if extra:
        out["again"] = step(1)
        L.vv_lm_attn(15)      # every A/B bit cleared: the kernel's first form (LmAttnArgs::variant 0)
        out["first_form"] = step(1)
        L.vv_lm_attn(1)
        out["kv_first_form"] = appended()
    return out


def _prefill(eng, xs, R):
    lens = _lens(R)
    slots = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(n) for n in lens]).to(**I32)
    last = (torch.cumsum(torch.tensor(lens), 0) - 1).to(**I32)
    eng.lm_forward(xs["prefill"], slots, pos, last)
    torch.cuda.synchronize()


@pytest.fixture(scope="module", params=["bf16", "w8"])
def runs(request):
    """Engine A (FP8 KV + the option; `w8`: FP8 weights + both options) prefilled, its rows
    read back, two decode steps; engine B (bf16 KV under vv_lm_attn_kvround(1), the same /
    the fake-quantised weights) filled with A's rows, the same steps; then C, that bf16
    engine as a plain one (the round trip off, its own prefill, step 1): its layer-0 appended
    rows.  Computed once."""
    w8 = request.param == "w8"
    gc.collect()
    L = _lib.lib()
    cfg = _cfg()
    sd = _spread_exponents(cfg, _sd(cfg, 82))
    g = torch.Generator().manual_seed(83)
    xs = {R: {"prefill": torch.randn(sum(_lens(R)), H, generator=g).bfloat16().to(dev),
              "step": [torch.randn(R, H, generator=g).bfloat16().to(dev) for _ in range(2)]} for R in ROWS}
    out = {"A": {}, "B": {}, "C": {}, "rows": {}}
    try:
        a = _engine(cfg, sd, 8, weight_dtype=FP8 if w8 else None, kv_dtype=FP8, lm_attn_kv8=True, lm_attn_w8=w8)
        assert a.weights_quantized() == w8 and L.vv_lm_attn_kv8(a.h) == 1
        for R in ROWS:
            _prefill(a, xs[R], R)
            out["rows"][R] = [tuple(t.cpu() for t in kv_read(a, r, 0, n)) for r, n in enumerate(_lens(R))]
            out["A"][R] = _steps(a, xs[R], R, True)
        a.check_sync()
        assert_counters_consistent(a)
        _close(a)
        b = _engine(cfg, fake_quantize_state_dict(sd, cfg) if w8 else sd, 8)
        assert not b.weights_quantized() and L.vv_kv_dtype(b.h) == 0
        L.vv_lm_attn_kvround(1)
        for R in ROWS:
            for r, (k, v) in enumerate(out["rows"][R]):
                kv_write(b, r, 0, k.shape[2], k, v)
            out["B"][R] = _steps(b, xs[R], R, True)
        L.vv_lm_attn_kvround(0)
        for R in ROWS:
            _prefill(b, xs[R], R)
            lens = _lens(R)
            ar = torch.arange(R).to(**I32)
            assert L.vv_lm_attn_active(b.h, R, max(lens) + 1) == 1
            b.lm_forward(xs[R]["step"][0], ar, torch.tensor(lens).to(**I32), ar)
            out["C"][R] = [tuple(t[0].cpu() for t in kv_read(b, r, n, n + 1)) for r, n in enumerate(lens)]
        b.check_sync()
        assert_counters_consistent(b)
        _close(b)
    finally:
        L.vv_lm_attn(1)
        L.vv_lm_attn_kvround(0)
    return out


def test_appended_rows_cover_several_binades(runs):
    """floor(log2(amax)) of the rows the decode steps appended (A's, dequantised)."""
    bins = set()
    for R in ROWS:
        for k, v in runs["A"][R]["kv"]:
            for t in (k, v):
                amax = t.view(torch.bfloat16).float().abs().amax(-1)
                assert (amax > 0).all()
                bins |= set(torch.floor(torch.log2(amax)).flatten().int().tolist())
    print("binades of the appended rows' amax:", sorted(bins))
    assert len(bins) >= 4 and min(bins) >= -8 and max(bins) <= 8, sorted(bins)   # test_gpu_kv8.py: randn rows times 2^-6 .. 2^6


@pytest.mark.parametrize("R", ROWS)
def test_bit_identical_to_the_round_trip_on_bf16(runs, R):
    A, B = runs["A"][R], runs["B"][R]
    for s in range(2):
        (h, lg), (hr, lgr) = A["steps"][s], B["steps"][s]
        assert torch.isfinite(lg).all() and torch.isfinite(h.view(torch.bfloat16).float()).all()
        print(f"R={R} step {s}: {(h != hr).sum().item()} of {h.numel()} hidden values differ from the round trip")
        assert torch.equal(h, hr) and torch.equal(lg, lgr)
    for r, ((k, v), (kr, vr)) in enumerate(zip(A["kv"], B["kv"])):
        print(f"R={R} row {r}: {(k != kr).sum().item()} K and {(v != vr).sum().item()} V values of the appended rows differ")
        assert k.any() and v.any() and torch.equal(k, kr) and torch.equal(v, vr)
    for run in (A, B):
        h, lg = run["steps"][1]
        for other in ("again", "first_form"):
            assert torch.equal(run[other][0], h) and torch.equal(run[other][1], lg), other
        assert all(torch.equal(x, y) for p, q in zip(run["kv_first_form"], run["kv"]) for x, y in zip(p, q))


@pytest.mark.parametrize("R", ROWS)
def test_quantiser_is_the_cpu_statement(runs, R):
    """A's layer-0 rows of step 1 == fake_quantize_kv of a plain bf16 engine's (they depend
    only on the input, the weights and the position)."""
    for r, ((k, v), (kc, vc)) in enumerate(zip(runs["A"][R]["kv"], runs["C"][R])):
        for name, got, ref in (("K", k, kc), ("V", v, vc)):
            want = bits(fake_quantize_kv(ref))          # [kv head][1][128], layer 0
            assert ref.float().abs().max() > 0
            assert torch.equal(got[0, :, :1], want), (R, r, name)


# ------------------------------------------------------------------ 3. several rows of one slot in one pass
def _multi_row_passes(eng, seed_rows, xs, one_launch=True):
    """From the given slot contents: one pass of 5 rows at positions 0..4 of slot 0; then one
    pass of 3 rows at positions 30, 31, 32 of slot 1 (30 keys) with a single row of slot 2 (7
    keys).  Hidden bits of every row and the appended rows."""
    for slot, (k, v) in seed_rows.items():
        kv_write(eng, slot, 0, k.shape[2], k, v)
    L = _lib.lib()
    out = []
    for slots, pos in (([0] * 5, [0, 1, 2, 3, 4]), ([1, 1, 1, 2], [30, 31, 32, 7])):
        n = len(slots)
        L.vv_lm_attn(1 if one_launch else 0)
        assert L.vv_lm_attn_active(eng.h, n, max(pos) + 1) == (1 if one_launch else 0)
        h, _ = eng.lm_forward(xs[n], torch.tensor(slots).to(**I32), torch.tensor(pos).to(**I32), torch.arange(n).to(**I32))
        torch.cuda.synchronize()
        rows = [tuple(bits(t) for t in kv_read(eng, s, p, p + 1)) for s, p in zip(slots, pos)]
        out.append((h.clone(), rows))
    L.vv_lm_attn(1)
    return out


def test_several_rows_of_one_slot_in_one_pass():
    L = _lib.lib()
    cfg = _cfg()
    sd = _spread_exponents(cfg, _sd(cfg, 84))
    g = torch.Generator().manual_seed(85)
    xs = {n: torch.randn(n, H, generator=g).bfloat16().to(dev) for n in (5, 4)}
    ex = torch.randint(-5, 6, (2, NKV, 30, 1), generator=g)
    raw = {1: (torch.ldexp(torch.randn(2, NKV, 30, HD, generator=g), ex).bfloat16(),
               torch.ldexp(torch.randn(2, NKV, 30, HD, generator=g), ex.flip(2)).bfloat16()),
           2: (torch.randn(2, NKV, 7, HD, generator=g).bfloat16(), torch.randn(2, NKV, 7, HD, generator=g).bfloat16())}
    a = _engine(cfg, sd, 2, kv_dtype=FP8, lm_attn_kv8=True)
    for slot, (k, v) in raw.items():
        kv_write(a, slot, 0, k.shape[2], k, v)
    deq = {slot: tuple(t.cpu() for t in kv_read(a, slot, 0, raw[slot][0].shape[2])) for slot in raw}   # B's cache = A's
    A = _multi_row_passes(a, deq, xs)
    a.check_sync()
    _close(a)
    b = _engine(cfg, sd, 2)
    L.vv_lm_attn_kvround(1)
    B = _multi_row_passes(b, deq, xs)
    L.vv_lm_attn_kvround(0)
    b.check_sync()
    _close(b)
    t = _engine(cfg, sd, 2, kv_dtype=FP8)          # a fresh FP8-KV engine: the three launches + k_kv_quant
    T = _multi_row_passes(t, deq, xs, one_launch=False)
    _close(t)
    for i, ((h, rows), (hb, rowsb), (ht, _)) in enumerate(zip(A, B, T)):
        assert torch.isfinite(h.float()).all()
        print(f"pass {i}: {(bits(h) != bits(hb)).sum().item()} hidden values differ from the round trip; "
              f"vs the three launches rel {rel_err(h, ht):.3e} cosine {cos(h, ht):.6f}")
        assert torch.equal(bits(h), bits(hb))
        for (k, v), (kb, vb) in zip(rows, rowsb):
            assert k.any() and v.any() and torch.equal(k, kb) and torch.equal(v, vb)
        assert rel_err(h, ht) < 2e-2 and cos(h, ht) > 0.999


# ------------------------------------------------------------------ 5. against the other paths
@pytest.mark.parametrize("n", [1, 3])
def test_decode_vs_three_launches_and_reference(n):
    L = _lib.lib()
    cfg = _cfg()
    sd = _sd(cfg, 86 + n)
    eng = _engine(cfg, sd, n, kv_dtype=FP8, lm_attn_kv8=True)
    R = 2 * n
    assert L.vv_lm_attn_active(eng.h, R, 64) == 1
    lcfg = dict(cfg.decoder_config)
    osd = {k[len(LMP):]: v for k, v in sd.items() if k.startswith(LMP)}
    g = torch.Generator().manual_seed(90 + n)
    lens = [5 + 3 * r for r in range(R)]
    xs = [torch.randn(m, H, generator=g).bfloat16() for m in lens]
    kvs = [olm.RowKV(2) for _ in lens]
    for r in range(R):
        kv8_ref.forward_rows(osd, lcfg, xs[r][None], kvs[r:r + 1], kv_hook=fake_quantize_kv)
    slots = torch.cat([torch.full((m,), r) for r, m in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(m) for m in lens]).to(**I32)
    last = torch.cumsum(torch.tensor(lens), 0) - 1
    eng.lm_forward(torch.cat(xs).to(dev), slots, pos, last.to(**I32))
    Lt = torch.tensor(lens)
    ar = torch.arange(R).to(**I32)
    for s in range(3):
        step_x = torch.randn(R, H, generator=g).bfloat16()
        ref = kv8_ref.forward_rows(osd, lcfg, step_x[:, None], kvs, kv_hook=fake_quantize_kv)[:, -1]
        L.vv_lm_attn(0)           # q|k|v, k_kv_quant, k_attn, o_proj on the same KV state (the step's own rows are rewritten below)
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
              f"vs the reference: rel {rel_err(one, ref):.3e} cosine {cos(one, ref):.6f}")
        assert rel_err(one, three) < 2e-2 and cos(one, three) > 0.999
        assert rel_err(one, ref) < 2e-2 and cos(one, ref) > 0.999
    eng.check_sync()
    assert_counters_consistent(eng)
    eng.close()


# ------------------------------------------------------------------ 6. generate() end to end
def test_generate_from_pretrained(tmp_path):
    L = _lib.lib()
    cfg = _cfg()
    write_synthetic_checkpoint(str(tmp_path), cfg, seed=88, mode="test")
    kw = dict(torch_dtype=torch.bfloat16, device_map="cuda", max_batch=1, max_ctx=MAX_CTX, kv_dtype=FP8)
    M = VibeVoiceForConditionalGenerationInference
    plain = M.from_pretrained(str(tmp_path), **kw)
    assert plain.lm_attn_kv8 is False and L.vv_lm_attn_active(plain.engine.h, 2, 64) == 0
    kv_bytes = plain.engine.kv_bytes()
    plain.engine.close()
    del plain
    gc.collect()
    m = M.from_pretrained(str(tmp_path), lm_attn_kv8=True, **kw)
    assert m.lm_attn_kv8 is True and m.engine.lm_attn_kv8 is True and L.vv_lm_attn_kv8(m.engine.h) == 1
    assert L.vv_lm_attn_active(m.engine.h, 2, 64) == 1          # generate()'s step shape at B = 1: 2 rows
    assert m.engine.kv_bytes() == kv_bytes
    m.set_ddpm_inference_steps(5)
    ids = torch.randint(0, 151000, (1, 12), generator=torch.Generator().manual_seed(3))
    mask = torch.ones(1, 12, dtype=torch.long)
    sched = [[D, D, D, E, S, D, X]]

    def run(graphs):
        torch.manual_seed(77)
        o = m.generate(input_ids=ids, attention_mask=mask, tokenizer=TK, cfg_scale=1.3, forced_tokens=sched,
                       use_graphs=graphs, show_progress_bar=False)
        return o.sequences.clone(), o.speech_outputs[0].clone()

    eager, graph = run(False), run(True)
    assert len(m._graph_cache) >= 1 and torch.isfinite(eager[1].float()).all() and eager[1].float().abs().max() > 0
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    m.engine.check_sync()
    assert_counters_consistent(m.engine)
    m.engine.close()
