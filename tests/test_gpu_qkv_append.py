"""The LM's q|k|v projection epilogue (EPI_ROPE: bias, bf16 rounding, RoPE on q
and k, q store, K append at [slot][kv_head][pos][128], V append into the
32-position blocked layout) against tests/qkv_ref.py, a CPU reference that is
not the code under test -- for every hand-written form of it: k_lm_attn's copy,
epi_rope under k_gemv1 (row-per-wave and item-per-thread prologues), k_gemv<2..4>,
k_gemvw, k_gemm<32|64>, k_gemm_big<1|2>, rope_qk8 / rope_v8 under k_gemm_xl, the
FP8-weight kernels, the FP8-KV staging path, each with the cos / sin table or
inline cosf / sinf.

Exact tier: inputs built so that no sum depends on its order (qkv_ref.exact_case);
q, K and V must equal the reference bit for bit, except the elements rotated by a
cos / sin within relative 2^-20 of a bf16 rounding midpoint (<= 0.2 % per test,
asserted), which must lie within one bf16 ulp of max(|v|, |rot v|).  A canary
(the whole cache synthetic-filled and snapshotted before the pass) proves that
nothing but the pass's rows was written.
Dense tier: seeded random operands against fp64; q / K within 3 ulp of
max(|v|, |rot v|), V within 1 ulp of the reference, rel L2 < 4e-3 per tensor.
Each test asserts the kernel it ran from the host-only launch plan
(vv_gemm_plan / vv_gemm_plan_w8, vv_lm_attn_active).

Engines have one decoder layer, so vv_diag_lm_qkv returns layer 0's q (k_lm_attn
writes q to the same workspace rows as the separate q|k|v launch, so q is checked
for that form too).  Under an FP8 KV cache that hook refuses, so those cases
check K and V only."""
import copy
import ctypes
import gc

import pytest
import torch

import qkv_ref as R
from gpu_util import kv_synthetic
from oracle import lm as olm
from tiny import tiny_dict
from vibevoice_amd import _lib
from vibevoice_amd.config import VibeVoiceConfig
from vibevoice_amd.engine import Engine
from vibevoice_amd.weights import (dequantize_rows, fake_quantize_kv, pack, quantize_rows_e4m3,
                                   synthetic_state_dict)

gpu = pytest.mark.gpu
dev = "cuda"
FP8 = "fp8_e4m3"
EPI_ROPE = 5
THETA, EPS = 1e6, 1e-6
LAYOUTS = {"1.5b": dict(hidden=1536, heads=12, kv_heads=2, inter=8960),
           "large": dict(hidden=3584, heads=28, kv_heads=4, inter=18944)}
# GemmKind words of vv_gemm_plan
GEMV1, GEMV, GEMVW, GEMM64, GEMM32, BIG1, BIG2, XL = 0, 1, 2, 4, 5, 6, 7, 8
CTX = 1088          # 17 x 64 keys: decode positions up to 1,087, within k_lm_attn's 4,096 keys
LONG = 65536


@pytest.fixture(autouse=True)
def _collect_engines():
    """As tests/test_gpu_lm.py: garbage engines still count as registered contexts."""
    gc.collect()
    yield


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(t):
    return t.contiguous().view(torch.int16)


def _case(layout, tier):
    s = LAYOUTS[layout]
    make = R.exact_case if tier == "exact" else R.dense_case
    return make(s["hidden"], s["heads"], s["kv_heads"], seed=11 if layout == "1.5b" else 12)


# ------------------------------------------------------------------ the reference itself (no GPU)
POS_CPU = list(range(0, 140)) + list(range(32760, 32776)) + list(range(64990, 65190)) + [65535]


def test_reference_rotation_equals_oracle():
    """qkv_ref.rope (fp64 cos / sin of the fp32 angle, explicit roundings) == oracle.lm's rotation (torch's fp32
    cos / sin, bf16 tensor arithmetic) bit for bit on 357 positions up to 65,535 -- outside the elements whose
    cos / sin sits within 2^-20 of a rounding midpoint (where two correctly-written cosines may round apart),
    which must agree within one ulp and are <= 0.2 % of all."""
    pos = torch.tensor(POS_CPU)
    g = torch.Generator().manual_seed(3)
    v = torch.randn(len(POS_CPU), 3, 128, generator=g).bfloat16()
    cos, sin, near = R.cos_sin(pos, THETA)
    got = R.rope(v, cos, sin)
    oc, os_ = olm.rope_cos_sin(pos, 128, THETA, torch.bfloat16)
    ref = v * oc[:, None, :] + olm._rot(v) * os_[:, None, :]
    excl = R.excluded(near, 3)
    same = bits(got) == bits(ref)
    share = excl.float().mean().item()
    print(f"reference vs oracle: excluded share {share:.5%}, unequal outside it {(~same & ~excl).sum().item()}")
    assert bool((same | excl).all())
    assert bool(((got.double() - ref.double()).abs() <= R.rope_tol(v))[excl].all())
    assert share <= 2e-3
    assert torch.equal(R.inv_freq(THETA), 1.0 / (THETA ** (torch.arange(0, 128, 2, dtype=torch.float) / 128)))


def test_reference_near_midpoint_rule():
    """The exclusion rule flags a value next to a bf16 midpoint and nothing else; ulp_bf16 is the issue's."""
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8 + 2.0 ** -18, 1.0, 0.75, 0.0,
                      -(0.5 + 2.0 ** -9)], dtype=torch.float64)
    assert R._near_midpoint(x).tolist() == [True, True, False, False, False, False, True]
    assert R.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.3, 0.0])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -9, 0.0]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_exact_construction(layout):
    """The exact tier's operands: every row 1-3 powers of two in distinct eighths of K, all rows distinct (a
    permutation of output columns changes the result), exactly representable as e4m3 codes x 2^e, and
    acc + bias usually not a bf16 value (the first rounding is exercised)."""
    s = LAYOUTS[layout]
    case = _case(layout, "exact")
    H = s["hidden"]
    assert bool(((case["norm"].float() >= 0.5) & (case["norm"].float() < 2)).all())
    rows = []
    for n in "qkv":
        W, b = case[n]
        nz = W != 0
        cnt = nz.sum(1)
        assert int(cnt.min()) >= 1 and int(cnt.max()) <= 3
        m, e = torch.frexp(W.float()[nz])
        assert bool((m.abs() == 0.5).all()) and int(e.min()) >= -2 and int(e.max()) <= 4      # +-2^s, |s| <= 3
        eighth = torch.arange(H)[None, :].expand_as(W)[nz] // (H // 8)
        owner = torch.arange(W.shape[0])[:, None].expand_as(W)[nz]
        assert torch.unique(owner * 8 + eighth).numel() == int(cnt.sum())                     # distinct eighths per row
        assert torch.equal(dequantize_rows(*quantize_rows_e4m3(W)), W)
        rows.append(W)
    allw = torch.cat(rows)
    assert torch.unique(allw, dim=0).shape[0] == allw.shape[0]
    x = R.sign_rows(40, H, seed=1)
    assert torch.unique(x, dim=0).shape[0] == 40
    ref = R.exact_ref(case, x, torch.arange(40), THETA, s["heads"], s["kv_heads"])
    a = x.double() * case["norm"].double()
    inexact = 0
    for n in "qkv":
        W, b = case[n]
        sm = (a @ W.double().t()).float() + b.float()
        inexact += (sm.bfloat16().float() != sm).float().mean().item() / 3
    print(f"{layout}: acc + bias is not a bf16 value for {inexact:.1%} of the outputs")
    assert inexact > 0.5 and ref["v"].float().abs().max() > 0


def test_position_sets_excluded_share():
    """The share of q / K elements under the exclusion rule for the position sets the GPU tests use."""
    for name, pos in (("decode", R.decode_positions(CTX)), ("runs", R.runs_300(CTX)[1]),
                      ("long", list(range(LONG - 300, LONG)) + [32767, 32768, 65000])):
        near = R.cos_sin(torch.tensor(pos), THETA)[2]
        print(f"{name}: {near.float().mean().item():.5%} of (position, frequency) pairs near a midpoint")
        assert near.float().mean().item() <= 2e-3


# ------------------------------------------------------------------ engines
_PACKED = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_packed():
    yield
    _PACKED.clear()


def _cfg(layout, max_pos=4096):
    d = tiny_dict(layers=1, vocab=1024, **LAYOUTS[layout])
    d["decoder_config"]["max_position_embeddings"] = max_pos
    return VibeVoiceConfig(copy.deepcopy(d))


def _packed(layout, tier, weight_dtype):
    """One packed weight set per (layout, tier, weight format): synthetic_state_dict with layer 0's
    input_layernorm and q/k/v projections overwritten (as make_engine of tests/test_gpu_lm.py does)."""
    key = (layout, tier, weight_dtype)
    if key not in _PACKED:
        cfg = _cfg(layout)
        sd = synthetic_state_dict(cfg, seed=7, device=dev, mode="test", with_acoustic_encoder=False)
        for k, v in R.state_dict_overrides(_case(layout, tier)).items():
            assert sd[k].shape == v.shape, k
            sd[k] = v.to(dev)
        with torch.cuda.device(0):
            _PACKED[key] = pack(sd, cfg, torch.device(dev, 0), weight_dtype=weight_dtype)
    return _PACKED[key]


def _engine(layout, tier, max_batch, max_ctx, weight_dtype=None, kv_dtype=None):
    eng = Engine(_cfg(layout, max(4096, max_ctx)), None, dev, max_batch=max_batch, max_ctx=max_ctx,
                 valid_ids=[0, 1, 2, 3], packed=_packed(layout, tier, weight_dtype), kv_dtype=kv_dtype)
    assert eng.weights_quantized() == (weight_dtype == FP8)
    return eng


def kv_read(eng, slot, p0, p1):
    nkv = eng.cfg.decoder_config.num_key_value_heads
    k = torch.empty(1, nkv, p1 - p0, 128, dtype=torch.bfloat16, device=dev)
    v = torch.empty_like(k)
    _lib.check(_lib.lib().vv_diag_kv_read(eng.h, slot, p0, p1, P(k), P(v)), "diag_kv_read")
    return k[0], v[0]


def read_q(eng, slots, pos):
    n, nh, nkv = len(pos), eng.cfg.decoder_config.num_attention_heads, eng.cfg.decoder_config.num_key_value_heads
    q = torch.empty(n, nh, 128, dtype=torch.bfloat16, device=dev)
    k, v = (torch.empty(n, nkv, 128, dtype=torch.bfloat16, device=dev) for _ in range(2))
    arr = ctypes.c_int * n
    _lib.check(_lib.lib().vv_diag_lm_qkv(eng.h, n, 0, arr(*slots), arr(*pos), P(q), P(k), P(v)), "diag_lm_qkv")
    torch.cuda.synchronize()
    return q.cpu(), k.cpu(), v.cpu()


def fill_canary(eng, nslots, max_ctx, fp8_kv):
    if not fp8_kv:
        kv_synthetic(eng, torch.arange(nslots, dtype=torch.int32, device=dev), 0, max_ctx, seed=17)
        torch.cuda.synchronize()
    else:       # the synthetic fill writes a bf16 cache only: seeded rows through the quantising write
        nkv = eng.cfg.decoder_config.num_key_value_heads
        g = torch.Generator(device=dev).manual_seed(17)
        for s in range(nslots):
            k, v = (torch.randn(1, nkv, max_ctx, 128, device=dev, generator=g).bfloat16() for _ in range(2))
            _lib.check(_lib.lib().vv_diag_kv_write(eng.h, s, 0, max_ctx, P(k), P(v)), "diag_kv_write")
    return [kv_read(eng, s, 0, max_ctx) for s in range(nslots)]


class Stats:
    def __init__(self):
        self.excl = self.total = 0
        self.worst = {}

    def note(self, name, val):
        self.worst[name] = max(self.worst.get(name, 0.0), float(val))


def check_exact(name, got, ref, st, excl=None, tol=None):
    """got == ref bit for bit; under `excl` within `tol` instead."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    same = bits(got) == bits(ref)
    if excl is None:
        bad = ~same
    else:
        bad = ~same & ~excl
        st.excl += int(excl.sum())
        st.total += excl.numel()
        d = (got.double() - ref.double()).abs()
        assert bool((d <= tol)[excl].all()), f"{name}: an excluded element is off by more than one ulp"
    if bool(bad.any()):
        idx = bad.nonzero()[:8].tolist()
        first = tuple(idx[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ in bits; first at "
                             f"{idx}: got {got[first].item()!r}, reference {ref[first].item()!r}")


def test_checker_flags_what_a_wrong_kernel_would_write():
    """check_exact on the CPU: the reference passes; a row rotated at the neighbouring position, q heads swapped, a
    one-bit flip outside the excluded elements, and an excluded element two ulps off all fail."""
    case = _case("1.5b", "exact")
    pos = torch.tensor(R.runs_300(CTX)[1])
    x = R.sign_rows(300, 1536, seed=2)
    ref = R.exact_ref(case, x, pos, THETA, 12, 2)
    assert bool(ref["k_excl"].any())
    check_exact("K", ref["k"].clone(), ref["k"], Stats(), ref["k_excl"], ref["k_tol"])
    off = R.exact_ref(case, x, pos + 1, THETA, 12, 2)
    swapped = ref["q"][:, [1, 0] + list(range(2, 12))]
    flip = ref["k"].clone()
    i = tuple((~ref["k_excl"]).nonzero()[5].tolist())
    flip[i] = (bits(flip[i].reshape(1)) ^ 1).view(torch.bfloat16)[0]
    far = ref["k"].clone()
    j = tuple(ref["k_excl"].nonzero()[0].tolist())
    far[j] = (far[j].double() + 2 * ref["k_tol"][j] + 2.0 ** -20).bfloat16()
    for name, got, key in (("pos+1", off["k"], "k"), ("heads", swapped, "q"), ("bit", flip, "k"), ("far", far, "k")):
        with pytest.raises(AssertionError):
            check_exact(name, got, ref[key], Stats(), ref[key + "_excl"], ref[key + "_tol"])


def check_dense(name, got, ref, tol, mult, st):
    d = (got.double() - ref.double()).abs()
    ratio = torch.where(tol > 0, d / tol.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, 1e9), d))
    rel = ((got.double() - ref.double()).norm() / ref.double().norm()).item()
    st.note(name + " max |err| / ulp", ratio.max())
    st.note(name + " rel L2", rel)
    print(f"  {name}: max |got - ref| = {ratio.max().item():.3f} ulp (bound {mult}), rel L2 {rel:.3e} (bound 4e-3)")
    assert torch.isfinite(got.float()).all()
    assert ratio.max().item() <= mult, name
    assert rel < 4e-3, name


def run_case(layout, tier, passes, expect, *, max_batch, max_ctx=CTX, hooks=(), weight_dtype=None, kv_dtype=None,
             seed=0):
    """Canary fill + snapshot, the passes (each (slots, positions)), then q per pass and the whole cache of every
    slot against the reference and the snapshot.  hooks: (name, args to set, args to restore) of tuning hooks,
    set before the engine is built and restored in `finally`.  expect(eng, rows, keys): asserts the kernel."""
    L = _lib.lib()
    s = LAYOUTS[layout]
    H, nh, nkv = s["hidden"], s["heads"], s["kv_heads"]
    case = _case(layout, tier)
    st = Stats()
    eng, undo = None, []
    try:
        for name, on, off in hooks:
            undo.append((name, off))
            assert getattr(L, name)(*on) == 0, name
        eng = _engine(layout, tier, max_batch, max_ctx, weight_dtype, kv_dtype)
        nslots = 2 * max_batch
        snap = fill_canary(eng, nslots, max_ctx, kv_dtype is not None)
        per_slot = {i: [] for i in range(nslots)}
        seen = set()
        for pi, (slots, pos) in enumerate(passes):
            n = len(pos)
            assert len(set(zip(slots, pos)) | seen) == n + len(seen) and max(pos) < max_ctx and max(slots) < nslots
            seen |= set(zip(slots, pos))
            if tier == "exact":
                x = R.sign_rows(n, H, seed=1000 * seed + pi)
                ref = R.exact_ref(case, x, torch.tensor(pos), THETA, nh, nkv)
            else:
                x = torch.randn(n, H, generator=torch.Generator().manual_seed(1000 * seed + pi)).bfloat16()
                ref = R.dense_ref(case, x, torch.tensor(pos), THETA, nh, nkv, EPS)
                assert ref["v"].float().abs().min() >= 2.0 ** -4            # qkv_ref.dense_case: no cancelled V element
            expect(eng, n, max(pos) + 1)
            eng.lm_forward(x.to(dev), torch.tensor(slots, dtype=torch.int32, device=dev),
                           torch.tensor(pos, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                           max_pos=max(pos))
            torch.cuda.synchronize()
            if kv_dtype is None:
                q = read_q(eng, slots, pos)[0]
                if tier == "exact":
                    check_exact(f"q (pass {pi})", q, ref["q"], st, ref["q_excl"], ref["q_tol"])
                else:
                    check_dense(f"q (pass {pi})", q, ref["q"], ref["q_tol"], 3, st)
            for i in range(n):
                per_slot[slots[i]].append((pos[i], pi, i))
            passes[pi] = (slots, pos, ref)
        for slot in range(nslots):
            k, v = kv_read(eng, slot, 0, max_ctx)
            rows = per_slot[slot]
            keep = torch.ones(max_ctx, dtype=torch.bool, device=dev)
            if rows:
                idx = torch.tensor([r[0] for r in rows], device=dev)
                keep[idx] = False
            # canary: everything that is not a row of a pass is untouched
            for nm, got, was in (("K", k, snap[slot][0]), ("V", v, snap[slot][1])):
                same = bits(got[:, keep]) == bits(was[:, keep])
                assert bool(same.all()), (f"slot {slot}: {int((~same).sum())} {nm} elements outside the passes' rows "
                                          f"changed; first (head, kept row, dim) {(~same).nonzero()[0].tolist()}")
            if not rows:
                continue
            gk, gv = k[:, idx].transpose(0, 1).cpu(), v[:, idx].transpose(0, 1).cpu()       # [rows, nkv, 128]
            pick = lambda key: torch.stack([passes[pi][2][key][i] for _, pi, i in rows])
            rk, rv = pick("k"), pick("v")
            if kv_dtype is not None:
                assert not bool(pick("k_excl").any()), "FP8-KV cases use positions without near-midpoint cos / sin"
                rk, rv = fake_quantize_kv(rk), fake_quantize_kv(rv)
            if tier == "exact":
                check_exact(f"K (slot {slot})", gk, rk, st, pick("k_excl"), pick("k_tol"))
                check_exact(f"V (slot {slot})", gv, rv, st)
            else:
                check_dense(f"K (slot {slot})", gk, rk, pick("k_tol"), 3, st)
                check_dense(f"V (slot {slot})", gv, rv, R.ulp_bf16(rv), 1, st)
        if tier == "exact":
            share = st.excl / max(1, st.total)
            print(f"  excluded (near-midpoint cos / sin) share: {st.excl} of {st.total} = {share:.5%}")
            assert share <= 2e-3
        else:
            print("  observed maxima:", {k_: f"{v_:.4g}" for k_, v_ in st.worst.items()})
    finally:
        for name, off in reversed(undo):
            getattr(L, name)(*off)
        if eng is not None:
            eng.close()
    return st


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(layout, M, xf, w8=False):
    s = LAYOUTS[layout]
    N, K = (s["heads"] + 2 * s["kv_heads"]) * 128, s["hidden"]
    out = (ctypes.c_int * 12)()
    fn = _lib.lib().vv_gemm_plan_w8 if w8 else _lib.lib().vv_gemm_plan
    assert fn(M, N, K, xf, int(xf == 1), 0, EPI_ROPE, 0, _cus(), out, 12) == 0
    return list(out)


def expect_gemm(layout, kind, mrep=None, rw=None, w8=None):
    """The separate q|k|v launch runs `kind` (xf = 1 up to 16 rows; above, the engine normalises separately)."""
    def f(eng, n, keys):
        assert _lib.lib().vv_lm_attn_active(eng.h, n, keys) == 0
        p = _plan(layout, n, 1 if n <= 16 else 0, w8 is not None)
        assert p[0] == kind, (n, p)
        if mrep is not None:
            assert p[1] == mrep, (n, p)
        if rw is not None:
            assert p[6] == rw, (n, p)
        if w8 is not None:
            assert p[11] == w8, (n, p)
    return f


def expect_lm_attn(eng, n, keys):
    assert _lib.lib().vv_lm_attn_active(eng.h, n, keys) == 1, (n, keys)


LM_ATTN_OFF = ("vv_lm_attn", (0,), (1,))
RW_OFF = ("vv_gemv_tune_rw", (99,), (0,))
TABLE_OFF = ("vv_rope_table", (0,), (1,))


def tune_big(mode):
    return ("vv_gemm_tune_big", (mode,), (-1,))


def decode_passes(n, max_ctx=CTX):
    """All nine decode positions, n rows per pass (one row per slot), then n consecutive rows from position 5
    in slot 1 (no octet aligned)."""
    P9 = R.decode_positions(max_ctx)
    passes = []
    if n >= len(P9):
        passes.append(R.layout_decode(n, max_ctx))
    else:
        for i in range(0, len(P9), n):
            chunk = P9[i:i + n]
            passes.append((list(range(len(chunk))), chunk))
    passes.append(R.layout_run(n, 5, slot=1))
    return passes


# ------------------------------------------------------------------ 1. exact tier
@gpu
@pytest.mark.parametrize("n,form,table", [(n, f, 1) for n in (1, 3, 16) for f in ("lm_attn", "gemv1_rw", "gemv1_item")] +
                         [(3, f, 0) for f in ("lm_attn", "gemv1_rw", "gemv1_item")])
def test_exact_decode_rows(n, form, table):
    """<= 16 rows of the 1.5B layout: k_lm_attn (the sole context's default), k_gemv1 with the row-per-wave and
    the item-per-thread norm prologue; cos / sin from the table and (3 rows) inline."""
    hooks = {"lm_attn": [], "gemv1_rw": [LM_ATTN_OFF], "gemv1_item": [LM_ATTN_OFF, RW_OFF]}[form]
    expect = expect_lm_attn if form == "lm_attn" else expect_gemm("1.5b", GEMV1, rw=1 if form == "gemv1_rw" else 0)
    run_case("1.5b", "exact", decode_passes(n), expect, max_batch=(n + 1) // 2, hooks=hooks + ([] if table else [TABLE_OFF]),
             seed=n)


@gpu
@pytest.mark.parametrize("n,kind,mrep,layout", [(17, GEMV, 2, "run0"), (40, GEMV, 3, "run5"), (64, GEMV, 4, "runs"),
                                                (70, GEMM32, None, "run5"), (200, GEMM64, None, "runs")])
def test_exact_mid_rows(n, kind, mrep, layout):
    """17 .. 200 rows of the 1.5B layout: k_rmsnorm + k_gemv<2..4>, k_gemm<32>, k_gemm<64> (epi_rope per lane)."""
    if layout == "run0":
        passes = [R.layout_run(n, 0)]
    elif layout == "run5":
        passes = [R.layout_run(n, 5)]
    else:       # four slots, run lengths in 137 : 45 : 3 : 115's spirit, one run ending at max_ctx - 1
        a, b = (n * 137) // 300, (n * 45) // 300
        passes = [R.layout_runs([(0, 3, a), (1, CTX - b, b), (2, 62, 3), (3, 65, n - a - b - 3)])]
    run_case("1.5b", "exact", passes, expect_gemm("1.5b", kind, mrep=mrep), max_batch=2, seed=n)


@gpu
@pytest.mark.parametrize("form,big,pack,table,layout", [
    ("xl", 7, 1, 1, "runs"), ("xl", 7, 1, 1, "run0"), ("xl", 7, 1, 1, "run5"), ("xl", 7, 1, 1, "permuted"),
    ("xl", 7, 0, 1, "runs"), ("xl", 7, 1, 0, "runs"),
    ("big2", 6, 1, 1, "runs"), ("big1", 5, 1, 1, "runs"), ("gemm", 0, 1, 1, "runs"), ("gemm", 0, 1, 1, "permuted")])
def test_exact_300_rows(form, big, pack, table, layout):
    """300 rows of the 1.5B layout on k_gemm_xl (rope_qk8 / rope_v8: the 16-byte V store and its scalar
    fallback; packed and row-major A rows; table and inline cos / sin), k_gemm_big<2>, k_gemm_big<1> and k_gemm.
    runs: four slots with slot changes mid-octet and one at an octet whose first position is 0 (mod 8);
    permuted: the same rows in a seeded order (octets start at aligned positions with other successors)."""
    slots, pos = R.runs_300(CTX)
    if layout == "run0":
        slots, pos = R.layout_run(300, 0)
    elif layout == "run5":
        slots, pos = R.layout_run(300, 5)
    elif layout == "permuted":
        slots, pos = R.permuted(slots, pos, seed=5)
        assert any(pos[m] % 8 == 0 and pos[m + 1] != pos[m] + 1 for m in range(0, 296, 8))
    else:
        assert pos[184] % 8 == 0 and slots[185] != slots[184] and pos[185] == pos[184] + 1
    kind = {"xl": XL, "big2": BIG2, "big1": BIG1, "gemm": GEMM64}[form]
    hooks = [tune_big(big), ("vv_norm_pack", (pack,), (1,))] + ([] if table else [TABLE_OFF])
    run_case("1.5b", "exact", [(slots, pos)], expect_gemm("1.5b", kind), max_batch=2, hooks=hooks, seed=300 + big)


@gpu
@pytest.mark.parametrize("n,kind", [(2, GEMV1), (24, GEMVW), (64, GEMVW)])
def test_exact_large_layout(n, kind):
    """VibeVoice-Large's layout (H 3,584, 28 q / 4 kv heads: 7 q heads per kv head, 288 weight tiles): k_gemv1 at
    2 rows, k_gemvw at 24 and 64."""
    if n == 2:
        passes = [([0, 1], [0, 33]), ([0, 1], [1000, CTX - 1]), R.layout_run(2, 31, slot=2)]
    else:
        a = n // 2
        passes = [R.layout_runs([(0, 5, a), (1, CTX - (n - a - 3), n - a - 3), (3, 62, 3)])]
    run_case("large", "exact", passes, expect_gemm("large", kind), max_batch=2, seed=n)


@gpu
@pytest.mark.parametrize("n,kind,w8", [(3, 3, 0), (40, GEMV, 1), (200, GEMM64, 1)])
def test_exact_fp8_weights(n, kind, w8):
    """weight_dtype fp8_e4m3 (the exact tier's weights are e4m3 codes x 2^e exactly): k_gemv_w8 at 3 rows, the W8
    instantiations of k_gemv<3> and k_gemm<64> above 16 rows."""
    for nm in "qkv":
        W = _case("1.5b", "exact")[nm][0]
        assert torch.equal(dequantize_rows(*quantize_rows_e4m3(W)), W)
    if n == 3:
        passes, mb = decode_passes(3), 2
    elif n == 40:
        passes, mb = [R.layout_run(n, 5)], 1
    else:
        passes, mb = [R.layout_runs([(0, 3, 91), (1, CTX - 45, 45), (2, 62, 3), (3, 65, 61)])], 2

    def expect(eng, rows, keys):
        assert _lib.lib().vv_lm_attn_active(eng.h, rows, keys) == 0
        p = _plan("1.5b", rows, 1 if rows <= 16 else 0, w8=True)
        assert p[11] == w8 and (w8 == 0 or p[0] == kind), (rows, p)
    run_case("1.5b", "exact", passes, expect, max_batch=mb, weight_dtype=FP8, seed=50 + n)


def _clean_positions(cands, n):
    """The first n of `cands` whose cos / sin are all clear of the rounding midpoints."""
    near = R.cos_sin(torch.tensor(cands), THETA)[2].any(1)
    keep = [p for p, bad in zip(cands, near.tolist()) if not bad]
    assert len(keep) >= n
    return keep[:n]


@gpu
@pytest.mark.parametrize("n,kind", [(3, GEMV1), (70, GEMM32)])
def test_exact_fp8_kv(n, kind):
    """kv_dtype fp8_e4m3 (the staging path: cos / sin rows gathered by position, k_kv_quant moves the rows): the
    cache read back == fake_quantize_kv of the reference K / V bit for bit, nothing else written.  Positions are
    the first of the list without a near-midpoint cos / sin, so the comparison has no excluded element."""
    if n == 3:
        cands = [0, 31, 32, 33, 63, 64, 1000, CTX - 1]
        passes = [([0, 1, 2], _clean_positions(cands, 3)), ([3, 1, 0], _clean_positions(cands[::-1], 3))]
        assert not set(zip(*passes[0])) & set(zip(*passes[1]))
    else:
        pos = _clean_positions(list(range(5, 200)), 67)                 # ascending, gaps where a position is skipped
        passes = [([0] * 40 + [1] * 27 + [2] * 3, pos + _clean_positions([CTX - 1, CTX - 2, CTX - 3, CTX - 4, 64, 63], 3))]
    run_case("1.5b", "exact", passes, expect_gemm("1.5b", kind), max_batch=2, kv_dtype=FP8, seed=70 + n)


@gpu
@pytest.mark.parametrize("case", ["decode", "run40", "run300_xl"])
def test_exact_long_context(case):
    """max_ctx 65,536 (the 64K configuration), one slot: decode rows at 32,767 / 32,768 / 65,000 / 65,535, a
    40-row and a 300-row (k_gemm_xl) run ending at 65,535 -- the frequency index and the cache offsets at large p."""
    hooks = []
    if case == "decode":
        passes, expect = [([0] * 4, [32767, 32768, 65000, 65535])], expect_gemm("1.5b", GEMV1)
    elif case == "run40":
        passes, expect = [R.layout_run(40, LONG - 40)], expect_gemm("1.5b", GEMV, mrep=3)
    else:
        passes, expect, hooks = [R.layout_run(300, LONG - 300)], expect_gemm("1.5b", XL), [tune_big(7)]
    run_case("1.5b", "exact", passes, expect, max_batch=1, max_ctx=LONG, hooks=hooks, seed=65)


# ------------------------------------------------------------------ 2. dense tier
@gpu
@pytest.mark.parametrize("layout,n,big", [("1.5b", 3, -1), ("1.5b", 40, -1), ("1.5b", 300, 7), ("1.5b", 300, 0),
                                          ("large", 24, -1)])
def test_dense_vs_fp64(layout, n, big):
    """Seeded random bf16 operands against fp64 rounded only where the spec rounds.  q / K: |got - ref| <=
    3 ulp_bf16(max(|v|, |rot v|)) (a one-ulp flip of v costs <= ulp(v) |c|, one of its rotated partner <=
    ulp(u) |s|, the re-rounded products and sum <= 1 ulp of the output between them); V: 1 ulp of the reference;
    rel L2 < 4e-3 per tensor (test_gpu_gemm.py's fused-RMSNorm bound).  Rows end at position 65,535."""
    if n == 3:
        passes = [([0, 0, 1], [65000, LONG - 1, 33])]
        expect = expect_gemm(layout, GEMV1)
    else:
        passes = [R.layout_run(n, LONG - n)]
        expect = expect_gemm(layout, {40: GEMV, 24: GEMVW}[n] if n < 300 else (XL if big == 7 else GEMM64))
    run_case(layout, "dense", passes, expect, max_batch=1, max_ctx=LONG, hooks=[tune_big(big)], seed=n + big)


# ------------------------------------------------------------------ 3. vv_kv_copy on a bf16 cache
@gpu
def test_kv_copy_bf16():
    """Two layers, two slots: every dst row == the snapshot's src row in every layer and head, K and V; all
    else unchanged.  Pairs cross the 32-position V blocks (0 -> 31, 31 -> 32, 33 -> 64, 5 -> 37, 5 -> 69) and
    one has src == dst.  One call per group of pairs, no pair reading a row an earlier one wrote."""
    d = tiny_dict(hidden=768, layers=2, heads=6, kv_heads=2, inter=256, vocab=1024)
    cfg = VibeVoiceConfig(copy.deepcopy(d))
    sd = synthetic_state_dict(cfg, seed=9, device="cpu", mode="test", with_acoustic_encoder=False)
    eng = Engine(cfg, sd, dev, max_batch=1, max_ctx=128, valid_ids=[0, 1, 2, 3])
    try:
        def read(slot):
            k = torch.empty(2, 2, 128, 128, dtype=torch.bfloat16, device=dev)
            v = torch.empty_like(k)
            _lib.check(_lib.lib().vv_diag_kv_read(eng.h, slot, 0, 128, P(k), P(v)), "diag_kv_read")
            return k, v
        kv_synthetic(eng, torch.arange(2, dtype=torch.int32, device=dev), 0, 128, seed=3)
        torch.cuda.synchronize()
        snap = [read(s) for s in (0, 1)]
        assert not torch.equal(snap[0][0][0], snap[0][0][1]) and not torch.equal(snap[0][0], snap[1][0])
        calls = [[(0, 31, 32), (1, 33, 64), (1, 5, 69)], [(0, 0, 31), (1, 31, 32), (0, 5, 37), (1, 7, 7)]]
        model = [[t.clone() for t in s] for s in snap]
        for pairs in calls:
            sl, src, dst = (torch.tensor(c, dtype=torch.int32, device=dev) for c in zip(*pairs))
            eng.kv_copy(sl, src, dst)
            torch.cuda.synchronize()
            for s, a, b in pairs:
                for w in (0, 1):
                    model[s][w][:, :, b] = snap[s][w][:, :, a]
        for s in (0, 1):
            k, v = read(s)
            assert torch.equal(bits(k), bits(model[s][0])) and torch.equal(bits(v), bits(model[s][1])), s
            assert not torch.equal(bits(k), bits(snap[s][0]))
    finally:
        eng.close()
