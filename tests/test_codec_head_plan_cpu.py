"""How a codec step and a diffusion sample pick their kernels, host side (no device work): the pure parts of the
two plans (engine.cpp codec_route / head_route, exported as vv_diag_codec_route / vv_diag_head_route) swept
against the tables of DESIGN.md ("How a codec step picks its kernels", "How a diffusion sample picks its
kernels"), restated here.
"""
import ctypes
import itertools
import os
import re

from vibevoice_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, WIDE, STAGE, BLOCKS, GEMMS = range(5)
PRE_NONE, PRE_CONVT, PRE_SCONV, PRE_STEM = range(4)
POST_NONE, POST_HEAD = 0, 1


def test_export_and_header():
    L = _lib.lib()
    product = open(os.path.join(ROOT, "include", "vibevoice_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "vibevoice_hip_diag.h")).read()
    for name, nargs in (("vv_diag_codec_route", 21), ("vv_diag_head_route", 14), ("vv_diag_codec_plan", 5),
                        ("vv_diag_head_plan", 4)):
        assert len(getattr(L, name).argtypes) == nargs
        assert any(e[0] == name for e in _lib.EXPORTS)
        assert re.search(r"^int %s\(" % name, diag, re.M) and name not in product
    assert L.vv_diag_codec_route(*([1] * 20), None) != 0
    assert L.vv_diag_head_route(*([1] * 13), None) != 0
    assert L.vv_diag_codec_plan(None, 0, 1, None, 64) != 0 and L.vv_diag_head_plan(None, 1, None, 11) != 0


def real_stages():
    """(decoder, i, nst, C, T, depth, ctx, rat, Cn, in_ch) of the real nets' stages, as tests/tiny.py builds them
    for ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32 (engine.cpp convnet_shape)."""
    ratios, enc_depths, nf, nst = (8, 5, 5, 4, 2, 2), (3, 3, 3, 3, 3, 3, 8), 32, 7
    out = []
    T, chans = 1, [nf << (nst - 1 - i) for i in range(nst)]
    for i in range(nst):                                   # decoder: latent (64 channels) -> audio
        rat = 1 if i == 0 else ratios[i - 1]
        T *= rat
        out.append((1, i, nst, chans[i], T, enc_depths[nst - 1 - i], 6, rat, chans[i - 1] if i else 0, 64))
    assert [s[4] for s in out] == [1, 8, 40, 200, 800, 1600, 3200]
    T, chans = 3200, [nf << i for i in range(nst)]
    for i in range(nst):                                   # encoder: audio (1 channel) -> features
        rat = 1 if i == 0 else ratios[nst - 1 - i]
        T = -(-T // rat)
        out.append((0, i, nst, chans[i], T, enc_depths[i], 6, rat, chans[i - 1] if i else 0, 1))
    assert [s[4] for s in out[nst:]] == [3200, 1600, 800, 200, 40, 8, 1]
    return out


def table_route(sw, shape, fits):
    """DESIGN.md's table: the first route whose condition holds, in priority order."""
    stage, wide, tile, fusion, persist = sw
    decoder, i, nst, C, T, depth, ctx, rat, Cn, in_ch = shape
    f_tile, f_wide, f_stage, f_block, f_mix = fits
    pre = PRE_NONE
    if i > 0 and rat == 2:
        if decoder and Cn == 2 * C:
            pre = PRE_CONVT
        if not decoder and C == 2 * Cn:
            pre = PRE_SCONV
    if not decoder and i == 0 and in_ch == 1:
        pre = PRE_STEM
    post = POST_HEAD if decoder and i == nst - 1 else POST_NONE
    rows = max(1, min(T, 2048 // C))
    if tile and f_tile and not (decoder and i == 0):
        own_pre = pre != PRE_STEM if i == 0 else pre == PRE_NONE
        return (TILE, pre, post, int(own_pre), 0, 0)
    if wide and persist and f_wide:
        return (WIDE, PRE_NONE, POST_NONE, 1, 0, 0)
    if stage and persist and f_stage:
        return (STAGE, PRE_NONE, POST_NONE, 1, 0, 0)
    if fusion & 2 and f_block:
        return (BLOCKS, PRE_NONE, POST_NONE, 1, 0, rows)
    return (GEMMS, PRE_NONE, POST_NONE, 1, int(bool(fusion & 1 and f_mix)), rows)


def test_codec_route_follows_the_table():
    L = _lib.lib()
    out = (ctypes.c_int * 6)()
    stages = real_stages()
    n = 0
    seen = set()
    for shape in stages:
        # (vv_codec_stage: bits 1..3 pick a weight-stream variant of the persistent launch; any bit is "on")
        for sw in itertools.product((0, 1, 4), (0, 1), (0, 1), (0, 1, 2, 3), (0, 1)):
            for fits in itertools.product((0, 1), repeat=5):
                out[:] = [-1] * 6
                assert L.vv_diag_codec_route(*sw, *shape, *fits, out) == 0
                got, want = tuple(out), table_route(sw, shape, fits)
                assert got == want, (sw, shape, fits, got, want)
                route, pre, post, own_pre, xf_mix, R = got
                decoder, i, nst = shape[:3]
                assert not (decoder and i == 0 and route == TILE)
                assert (post == POST_HEAD) == (route == TILE and decoder and i == nst - 1)
                if route == TILE and pre in (PRE_CONVT, PRE_SCONV, PRE_STEM):
                    assert own_pre == 0
                if i == 0:
                    assert own_pre == (0 if not decoder and route == TILE and pre == PRE_STEM else 1)
                if route != TILE:
                    assert (pre, post, own_pre) == (PRE_NONE, POST_NONE, 1)
                assert (R > 0) == (route in (BLOCKS, GEMMS)) and (not xf_mix or route == GEMMS)
                seen.add(route)
                n += 1
    assert n == 14 * (3 * 2 * 2 * 4 * 2) * 32 and seen == {TILE, WIDE, STAGE, BLOCKS, GEMMS}
    # the transitions the real nets fuse into a tile launch, all fits answering yes
    pres = [table_route((1, 1, 1, 3, 1), s, (1,) * 5)[1] for s in stages]
    assert pres[:7] == [PRE_NONE] * 5 + [PRE_CONVT] * 2 and pres[7:] == [PRE_STEM, PRE_SCONV, PRE_SCONV] + [PRE_NONE] * 4


def table_head(head_tp, head_gemv, tp_size, comm, m16, m16_pre, fin, persist, steps, R, wbytes, f_m16, f_fin):
    """DESIGN.md's table for a sample of R rows."""
    keep = wbytes <= 192 << 20 and not (head_tp and tp_size > 1)
    sharded = head_tp and (tp_size > 1 or comm)
    one = m16 != 0 and not head_tp and head_gemv and f_m16 and persist
    pre = one and m16_pre and R > 4
    a_first = True if m16 & 2 else False if m16 & 8 else R > 8
    late_down = not m16 & 4
    fused = fin and not head_tp and keep and f_fin and steps >= 3
    nfused = (steps - 1) // 2 * 2 if fused else 0
    return tuple(int(bool(v)) if isinstance(v, bool) else v for v in
                 (R, bool(keep), bool(sharded), bool(one), bool(pre), a_first, bool(late_down), bool(fused), nfused,
                  steps - 1 - nfused, R <= 16))


def test_head_route_follows_the_table():
    L = _lib.lib()
    out = (ctypes.c_int * 11)()
    small = 4 * 3 * 4608 * 1536 * 2                       # the 1.5B head's layers: 170 MB
    n = 0
    for R, steps, head_tp, head_gemv, persist, m16, m16_pre, fin, f_m16, f_fin in itertools.product(
            (2, 4, 6, 16, 18), (1, 2, 3, 4, 10), (0, 1), (0, 1), (0, 1), range(16), (0, 1), (0, 1), (0, 1), (0, 1)):
        for tp_size, comm, wbytes in ((1, 0, small), (1, 1, small), (4, 1, small), (1, 0, 193 << 20)):
            args = (head_tp, head_gemv, tp_size, comm, m16, m16_pre, fin, persist, steps, R, wbytes, f_m16, f_fin)
            out[:] = [-1] * 11
            assert L.vv_diag_head_route(*args, out) == 0
            got = tuple(out)
            assert got == table_head(*args), (args, got, table_head(*args))
            _, keep, sharded, one, pre, a_first, late_down, fused, nfused, s0, epi = got
            assert not pre or (R > 4 and one)
            assert a_first == (1 if m16 & 2 else 0 if m16 & 8 else int(R > 8))
            assert late_down == (0 if m16 & 4 else 1)
            assert nfused % 2 == 0 and 0 <= nfused <= steps - 1 and s0 == steps - 1 - nfused
            if steps < 3 or sharded:
                assert nfused == 0 and not fused
            assert (nfused > 0) == bool(fused)
            assert epi == int(R <= 16)
            n += 1
    assert n == 5 * 5 * 2 * 2 * 2 * 16 * 2 * 2 * 2 * 2 * 4
