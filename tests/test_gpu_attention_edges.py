"""k_attn, its three merges (the in-kernel ticket merge, k_attn_merge, the deferred / grouped consumer) and
k_attn_pf against the fp64 reference of tests/attn_ref.py, per (row, head): planted keys at every index
where the split plan hands work over (attn_ref.split_edges), keys planted past a row's last, a NaN tail,
and staircases that move the running max.  tests/test_attn_edges_cpu.py shows from the reference alone
that each case here sees a dropped or an extra key as rel >= 0.2 and that the declared roundings use at
most a third of the bound, so a failure here is the kernel's.

Every raw cache below carries one spare head of zeros behind its last head, so no launch can read outside
an allocation."""
import ctypes
import gc
import math

import pytest
import torch

import attn_ref as ar
from tests_engine import tiny_engine
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
dev = "cuda"
I32 = dict(dtype=torch.int32, device=dev)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int16)


def _padded(x):
    """x [slot][kv head][...] flat on the device, one spare head of zeros behind it."""
    n = x.numel()
    buf = torch.zeros(n + n // (x.shape[0] * x.shape[1]), dtype=torch.bfloat16, device=dev)
    buf[:n] = x.reshape(-1).to(dev)
    return buf


def launch(case, K=None, V=None):
    """vv_attention_bf16 over the case's raw cache (V in the engine's blocks of [128 dims][32 positions])."""
    K, V = case.K if K is None else K, case.V if V is None else V
    nslot, nkv, ctx, _ = K.shape
    kb = _padded(K)
    vb = _padded(V.view(nslot, nkv, ctx // 32, 32, 128).transpose(3, 4).contiguous())
    q = case.q.to(dev)
    out = torch.full_like(q, math.nan)
    slots, pos = torch.tensor(case.slots, **I32), torch.tensor(case.pos, **I32)
    rc = _lib.lib().vv_attention_bf16(case.nq, case.nh, case.nkv, P(q), P(kb), P(vb), nkv * ctx * 128, ctx * 128, P(slots),
                                      P(pos), max(case.pos) + 1, P(out), tiny_engine().h, stream())
    _lib.check(rc, "attention")
    torch.cuda.synchronize()
    return out


def check(out, case, what, ref=None):
    errs = ar.head_errs(out.float().cpu(), case.ref() if ref is None else ref)
    e, i, h = ar.worst(errs)
    print(f"{case.tag}, {what}: worst (row, head) rel {e:.3e} at row {i} (pos {case.pos[i]}, aimed at {int(case.aim[i, h])}) head {h}")
    assert torch.isfinite(out.float()).all(), (case.tag, what)
    assert e < ar.BOUND, (case.tag, what, e, i, h)
    return e


class tuned:
    def __init__(self, chunk, merge_in):
        self.args = (chunk, merge_in)

    def __enter__(self):
        _lib.check(_lib.lib().vv_attn_tune(*self.args), "attn_tune")

    def __exit__(self, *exc):
        _lib.lib().vv_attn_tune(0, -1)


class prefill:
    def __enter__(self):
        _lib.lib().vv_attn_prefill(1)

    def __exit__(self, *exc):
        _lib.lib().vv_attn_prefill(-1)


# ------------------------------------------------------------------ k_attn and its merges, raw cache
@pytest.mark.parametrize("nh,nkv", ar.LAYOUTS)
@pytest.mark.parametrize("plan", list(ar.DECODE_PLANS))
def test_decode_plan_edges(plan, nh, nkv):
    """Per plan of attn_ref.DECODE_PLANS: rows aimed at every split, wave, step and register-set edge, rows
    aimed at keys past their last (pos + 1, pos + 8, the end of the loaded 8-key V group, the next step),
    then the same launch with bf16 NaN in K and V from the longest row's end to capacity (attn_dev.h
    "Tail masking": clamped K loads, V masked by a select)."""
    chunk, merges, _, _ = ar.DECODE_PLANS[plan]
    case = ar.decode_case(plan, nh, nkv)
    Kn, Vn = ar.poisoned(case)
    for merge_in in merges:
        with tuned(chunk, merge_in):
            check(launch(case), case, f"merge_in {merge_in}")
            check(launch(case, Kn, Vn), case, f"merge_in {merge_in}, NaN tail")


@pytest.mark.parametrize("step_nats,direction,nsteps", ar.STAIRCASES)
def test_decode_staircases(step_nats, direction, nsteps):
    """256 keys whose per-step max rises by 9 or 4 nats or falls by 9: 32-key splits merged in the kernel and
    by k_attn_merge (weights e^{m_s - M} down to e^-63), and the default plan's eight waves merged in LDS."""
    case = ar.stair_case(step_nats, direction, nsteps)
    for chunk, merge_in in ar.STAIR_PLANS:
        with tuned(chunk, merge_in):
            check(launch(case), case, f"plan ({chunk}, {merge_in})")


def test_decode_staircase_carried():
    """1,024 keys rising by 2 nats per step under the default plan: four carried steps per wave, each with
    alpha = e^-2 on l and O (attn_step<.., true>), then the eight waves' LDS merge."""
    case = ar.stair_case(*ar.GENTLE)
    check(launch(case), case, "default plan")


# ------------------------------------------------------------------ an engine's cache: forms 0, 2, 3 and FP8
def _attend(eng, case, form):
    q = case.q.to(dev)
    out = torch.full_like(q, math.nan)
    slots, pos = torch.tensor(case.slots, **I32), torch.tensor(case.pos, **I32)
    _lib.check(_lib.lib().vv_diag_attn_ctx(eng.h, 0, case.nq, P(q), P(slots), P(pos), form, P(out), stream()), "diag_attn_ctx")
    torch.cuda.synchronize()
    return out


def _kv_write(eng, K, V):
    _lib.check(_lib.lib().vv_diag_kv_write(eng.h, 0, 0, K.shape[2], P(K.contiguous()), P(V.contiguous())), "diag_kv_write")


def test_engine_forms_and_fp8_cache():
    """The planted rows over an engine's own cache (1 layer, max_ctx 1,280, 160-key splits: 8 splits of 4
    waves, two steps per wave) through vv_diag_attn_ctx: the deferred merge equals the in-kernel one bit
    for bit, the grouped one is within the bound; then an FP8-KV engine against a bf16 engine holding its
    dequantised rows: bit-equal outputs, and the bound against the reference over those rows."""
    case, _ = ar.engine_case()
    cfg = tiny_config(hidden=1536, layers=1, heads=12, kv_heads=2, inter=256)
    sd = synthetic_state_dict(cfg, seed=5, device="cpu", mode="test", with_acoustic_encoder=False)
    gc.collect()
    b16 = Engine(cfg, sd, dev, max_batch=1, max_ctx=ar.ENGINE_CTX)
    q8 = Engine(cfg, sd, dev, max_batch=1, max_ctx=ar.ENGINE_CTX, kv_dtype="fp8_e4m3")
    try:
        with tuned(ar.ENGINE_CHUNK, -1):
            _kv_write(b16, case.K.to(dev), case.V.to(dev))
            inker, defer, group = (_attend(b16, case, form) for form in (0, 2, 3))
            check(inker, case, "in-kernel merge")
            assert torch.equal(bits(defer), bits(inker))
            check(group, case, "grouped merge")
            check(group, case, "grouped against the in-kernel merge", ref=inker.float().cpu().reshape(case.nq, case.nh, 128))
            # FP8: what the cache holds, read back, is the bf16 engine's cache and the reference's input
            _kv_write(q8, case.K.to(dev), case.V.to(dev))
            kd, vd = torch.empty_like(case.K, device=dev), torch.empty_like(case.V, device=dev)
            _lib.check(_lib.lib().vv_diag_kv_read(q8.h, 0, 0, ar.ENGINE_CTX, P(kd), P(vd)), "diag_kv_read")
            _kv_write(b16, kd, vd)
            deq = case.with_kv(kd.cpu(), vd.cpu())
            for form, name in ((0, "in-kernel merge"), (2, "deferred merge")):
                o8, o16 = _attend(q8, deq, form), _attend(b16, deq, form)
                assert torch.equal(bits(o8), bits(o16)), name
                check(o8, deq, f"FP8 cache, {name}")
    finally:
        b16.close()
        q8.close()


# ------------------------------------------------------------------ k_attn_pf
def _nan_from(case, first):
    K, V = case.K.clone(), case.V.clone()
    K[:, :, first:] = math.nan
    V[:, :, first:] = math.nan
    return K, V


@pytest.mark.parametrize("nh,nkv", ar.PREFILL_LAYOUTS)
def test_prefill_causal_edges(nh, nkv):
    """200 rows of one slot's causal prefill (QW = 1, QW = 2 and G = 1 forms), each aimed at key 0, its
    diagonal key, the one before, either side of its last step edge -- or at p + 1, the next row's key,
    written and excluded by the causal mask alone.

    Past nk = 200 the cache holds planted keys (200 in the last computed block, 224 in the stage's second
    block) and is then NaN.  NaN there is in contract, read off the kernel: the diagonal steps pick every
    score with a select (`in && key <= qpos ? s : -inf`, so a NaN score of a key past the row never
    reaches the max or P), the `k0 + 32 > nk` bit mask zeroes V past nk in the last computed block, and
    the stage's second block is not computed at all (`break`), only fetched -- which is why the context
    must be a multiple of 64 (test_prefill_needs_64_key_contexts)."""
    case = ar.prefill_causal_case(nh, nkv)
    with prefill():
        check(launch(case), case, "planted past nk")
        check(launch(case, *_nan_from(case, 200)), case, "NaN past nk")


@pytest.mark.parametrize("nh,nkv", [(12, 2), (28, 4)])
def test_prefill_staircases(nh, nkv):
    """64 rows at positions 192 .. 255 over 8 steps: rising by 9 nats moves the lazy max (PF_LAZY = 8 log2
    units) on every step, by 4 on alternate steps (P reaches 2^5.8 in between), falling by 9 never again --
    checked here from the reference's scores, then the kernel against the reference."""
    wants = (lambda n: list(range(n)), lambda n: list(range(0, n, 2)), lambda n: [0])
    for (step_nats, direction, _), want in zip(ar.STAIRCASES, wants):
        case = ar.prefill_stair_case(step_nats, direction, nh, nkv)
        moves = ar.lazy_max_moves(case)
        for i, p in enumerate(case.pos):
            seen = sum(1 for e in case.keys if e <= p)
            assert all(moves[i][h] == want(seen) for h in range(nh)), (case.tag, p)
        with prefill():
            check(launch(case), case, "k_attn_pf")


def test_prefill_tile_over_two_slots():
    """One tile, two slot passes: every aimed-at key is planted in the other slot too, along the same
    direction with another V (the CPU test shows a swapped slot as rel >= 0.2)."""
    case = ar.prefill_two_slot_case()
    with prefill():
        check(launch(case), case, "k_attn_pf")


def test_prefill_continuation_chunk():
    """Positions 500 .. 569 over 500 earlier keys: planted keys in the steps every row attends in full
    (no mask), at the last of them, and on the diagonal steps; planted keys, then NaN, past nk = 570."""
    case = ar.prefill_continuation_case()
    with prefill():
        check(launch(case), case, "planted past nk")
        check(launch(case, *_nan_from(case, 570)), case, "NaN past nk")


def test_prefill_needs_64_key_contexts():
    """k_attn_pf fetches whole 64-key stages, so over a context of 32 mod 64 its last stage would read 32
    keys past the head -- for the last head of the last slot, past the cache.  The launch is refused."""
    rows = [(0, p, [p // 2] * 12) for p in range(96)]
    case = ar.build_case("prefill, 96-key context", 12, 2, 1, 96, rows, seed=96)
    with prefill():
        with pytest.raises(RuntimeError, match="64"):
            launch(case)
    check(launch(case), case, "the decode kernel serves it")
