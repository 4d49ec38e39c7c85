"""The cases of tests/test_gpu_attention_edges.py judge the kernel and nothing else: from the fp64
reference alone (tests/attn_ref.py), every case is shown to

  detect    zeroing the key a (row, head) is aimed at changes that head's output by rel >= 0.2, twenty
            times the bound; taking in a planted key from past the row's last changes it by >= 0.2;
  leave headroom    the kernels' declared roundings (attention_emulated) cost at most a third of the bound
            on every (row, head), so a failure on the device is the kernel's;
  cover     every index of split_edges of every plan is aimed at by some (row, head) of that length, and
            the plan arithmetic restated in attn_ref agrees with the library's (vv_diag_attn_row_splits).

If a case exceeds a third of the bound the case changes, never the bound."""
import ctypes

import pytest
import torch

import attn_ref as ar
from vibevoice_amd import _lib
from vibevoice_amd.weights import fake_quantize_kv

DETECT = 0.2
HEADROOM = ar.BOUND / 3


def _check_case(case):
    ref = case.ref()
    assert torch.isfinite(ref).all()
    emu = ar.attention_emulated(case.q, case.K, case.V, case.slots, case.pos, case.nh, case.nkv)
    e, i, h = ar.worst(ar.head_errs(emu, ref))
    print(f"{case.tag}: {case.nq} rows, declared roundings cost at most {e:.2e} (row {i} head {h})")
    assert e <= HEADROOM, (case.tag, e, i, h)
    inside, past = case.inside(), case.past()
    if inside.any():
        gone = ar.attention_ref(case.q, case.K, case.V, case.slots, case.pos, case.nh, case.nkv,
                                zero=case.aim.masked_fill(~inside, -1))
        d = ar.head_errs(gone, ref)[inside]
        print(f"{case.tag}: without its aimed-at key a head changes by {float(d.min()):.3f} .. {float(d.max()):.3f}")
        assert float(d.min()) >= DETECT, case.tag
    if past.any():
        more = ar.attention_ref(case.q, case.K, case.V, case.slots, case.pos, case.nh, case.nkv,
                                include=case.aim.masked_fill(~past, -1))
        d = ar.head_errs(more, ref)[past]
        print(f"{case.tag}: with the planted key past its last a head changes by {float(d.min()):.3f} .. {float(d.max()):.3f}")
        assert float(d.min()) >= DETECT, case.tag


def _check_coverage(case, lens_edges):
    pos = torch.tensor(case.pos)
    for length, edges in lens_edges:
        aimed = set(case.aim[pos == length - 1].reshape(-1).tolist())
        missing = [e for e in edges if e not in aimed]
        assert not missing, (case.tag, length, missing)
        assert edges[0] == 0 and edges[-1] == length - 1


def _check_plan_arithmetic(lens_edges, nsplit, chunk):
    f = _lib.lib().vv_diag_attn_row_splits
    out = (ctypes.c_int * 3)()
    for length, edges in lens_edges:
        for group in (0, 2):
            assert f(length, nsplit, chunk, group, out) == 0
            assert (out[0], out[1], out[2]) == ar.row_splits(length, nsplit, chunk, group), (length, nsplit, chunk)
        assert f(length, nsplit, chunk, 0, out) == 0
        for s in range(out[1]):     # the library's splits begin and end on edges
            assert s * out[0] in edges and min(length, (s + 1) * out[0]) - 1 in edges


@pytest.mark.parametrize("nh,nkv", ar.LAYOUTS)
@pytest.mark.parametrize("plan", list(ar.DECODE_PLANS))
def test_decode_plans(plan, nh, nkv):
    case = ar.decode_case(plan, nh, nkv)
    chunk, _, lens, _ = ar.DECODE_PLANS[plan]
    assert [n for n, _ in case.lens_edges] == list(lens)
    assert case.past().any() and max(case.pos) + 1 + 32 <= case.ctx
    _check_coverage(case, case.lens_edges)
    _check_plan_arithmetic(case.lens_edges, case.nsplit, case.chunk)
    _check_case(case)


def test_plans_reach_what_they_name():
    """The shapes the plan table promises, from split_edges' own arithmetic."""
    def waves(length, nsplit, chunk):      # per split: the key counts of its waves
        ch, nact, _ = ar.row_splits(length, nsplit, chunk)
        nw, res = ar.plan_waves(chunk), []
        for s in range(nact):
            k0, k1 = s * ch, min(length, (s + 1) * ch)
            per = (-(-(k1 - k0) // nw) + 31) // 32 * 32
            res.append([max(0, min(k1, k0 + (w + 1) * per) - (k0 + w * per)) for w in range(nw)])
        return res
    assert waves(1000, 1, 1024) == [[128] * 7 + [104]]                 # four steps per wave, an 8-key tail
    assert waves(1025, 2, 1024)[1] == [1] + [0] * 7                    # a 1-key split
    assert waves(254, 8, 32)[-1] == [30, 0] and len(waves(97, 8, 32)) == 4
    assert waves(161, 2, 96)[1] == [64, 1] and waves(190, 2, 96)[1] == [64, 30]
    assert waves(700, 6, 128)[-1] == [32, 28, 0, 0]                    # waves with no key
    assert waves(1500, 6, 256)[0] == [32] * 8
    assert [ar.row_splits(n, 256, 32)[1] for n in (257, 513, 1280, 8192)] == [9, 17, 40, 256]
    assert len(waves(1280, 8, 160)) == 8 and waves(1280, 8, 160)[0] == [64, 64, 32, 0]
    assert waves(161, 8, 160)[1] == [1, 0, 0, 0]


@pytest.mark.parametrize("step_nats,direction,nsteps", ar.STAIRCASES + [ar.GENTLE])
def test_staircases(step_nats, direction, nsteps):
    case = ar.stair_case(step_nats, direction, nsteps)
    _check_case(case)
    # the graded scores are what the case says: the step maxima differ by step_nats (in nats)
    q = case.q.reshape(case.nq, case.nh, ar.HD).double()
    sc = (case.K.double()[0, 0] @ q[0, 0]) / ar.HD ** 0.5
    mx = torch.stack([sc[k0:k0 + 32].max() for k0 in range(0, 32 * nsteps, 32)])
    assert torch.allclose(mx[1:] - mx[:-1], torch.full((nsteps - 1,), float(direction * step_nats), dtype=torch.float64),
                          atol=0.02 * step_nats * nsteps)


def test_engine_case_and_its_fp8_image():
    case, lens_edges = ar.engine_case()
    _check_coverage(case, lens_edges)
    _check_plan_arithmetic(lens_edges, ar.plan_nsplit(ar.ENGINE_CTX, ar.ENGINE_CHUNK), ar.ENGINE_CHUNK)
    ns = ar.plan_nsplit(ar.ENGINE_CTX, ar.ENGINE_CHUNK)
    assert 2 <= ns <= 8                                                 # the deferred merge's range
    _check_case(case)
    # what an FP8 cache holds for it (weights.fake_quantize_kv == the device's quantiser, tests/test_gpu_kv8.py)
    _check_case(case.with_kv(fake_quantize_kv(case.K), fake_quantize_kv(case.V)))


@pytest.mark.parametrize("nh,nkv", ar.PREFILL_LAYOUTS)
def test_prefill_causal(nh, nkv):
    case = ar.prefill_causal_case(nh, nkv)
    assert case.ctx % 64 == 0 and case.past().any()
    pos = torch.tensor(case.pos)
    rows = case.aim[:, 0]
    for name, want in (("key 0", torch.zeros_like(pos)), ("the diagonal key", pos), ("the key before it", pos - 1),
                       ("the last step edge", 32 * (pos // 32)), ("the key before that edge", 32 * (pos // 32) - 1),
                       ("the next row's key", pos + 1)):
        assert int((rows == want).sum()) >= 20, name
    _check_case(case)


def test_prefill_staircases_move_the_lazy_max():
    """Rising by 9 nats (13 log2 units) moves k_attn_pf's lazy max on every step that holds a planted key
    the row sees, rising by 4 (5.8) on alternate ones, falling never after the first."""
    for (step_nats, direction, _), want in zip(ar.STAIRCASES, (lambda n: list(range(n)), lambda n: list(range(0, n, 2)),
                                                              lambda n: [0])):
        case = ar.prefill_stair_case(step_nats, direction)
        _check_case(case)
        moves = ar.lazy_max_moves(case)
        for i, p in enumerate(case.pos):
            seen = sum(1 for e in case.keys if e <= p)
            assert seen >= 7
            for h in range(case.nh):
                assert moves[i][h] == want(seen), (case.tag, p, h, moves[i][h])


def test_prefill_two_slots_and_continuation():
    two = ar.prefill_two_slot_case()
    assert two.nq == 32 and set(two.slots) == {0, 1}
    # a row's aimed-at key is planted in the other slot as well, along the same direction, with another V
    for i in range(two.nq):
        e, s = int(two.aim[i, 0]), two.slots[i]
        assert torch.equal(two.K[s, :, e], two.K[1 - s, :, e]) and not torch.equal(two.V[s, :, e], two.V[1 - s, :, e])
    _check_case(two)
    # ... so reading the other slot is seen: the reference over swapped slots differs by far more than the bound
    swapped = ar.attention_ref(two.q, two.K.flip(0), two.V.flip(0), two.slots, two.pos, two.nh, two.nkv)
    assert float(ar.head_errs(swapped, two.ref()).min()) >= DETECT
    cont = ar.prefill_continuation_case()
    kfull = min(cont.pos) + 1
    assert int((cont.aim[:, 0] < kfull - 32).sum()) >= 20 and int((cont.aim[:, 0] >= 480).sum()) >= 20
    _check_case(cont)


def test_pooled_norm_hides_the_long_row():
    """Why no bound here is pooled: [65000, 3] keys of randn (the 64K case of tests/test_gpu_attention.py
    with 4 / 2 heads for its 12 / 2), the long row's output replaced by zeros -- rel 1.0 on each of its
    heads -- is under 1e-2 pooled."""
    g = torch.Generator().manual_seed(0)
    lens, nh, nkv = [65000, 3], 4, 2
    K = torch.randn(2, nkv, max(lens), ar.HD, generator=g).bfloat16()
    V = torch.randn(2, nkv, max(lens), ar.HD, generator=g).bfloat16()
    q = torch.randn(2, nh * ar.HD, generator=g).bfloat16()
    ref = ar.attention_ref(q, K, V, [0, 1], [n - 1 for n in lens], nh, nkv)
    out = ref.clone()
    out[0] = 0
    pooled, per_head = ar.pooled_err(out, ref), ar.head_errs(out, ref)
    print(f"long row zeroed: pooled rel {pooled:.4f}, its heads {float(per_head[0].min()):.3f}")
    assert pooled < 1e-2 and float(per_head[0].min()) == 1.0 and float(per_head[1].max()) == 0.0
    emu = ar.attention_emulated(q, K, V, [0, 1], [n - 1 for n in lens], nh, nkv)
    assert ar.worst(ar.head_errs(emu, ref))[0] <= HEADROOM
