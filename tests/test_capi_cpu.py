"""CPU-side checks of the C ABI library: it builds, loads and exports every
entry point declared in include/vibevoice_hip.h (the product interface) and
include/vibevoice_hip_diag.h (kernel entry points, tuning hooks, stamps), and
the product header declares none of the diagnostics (no GPU compute here)."""
import ctypes
import os
import re

from vibevoice_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(headers=("vibevoice_hip.h", "vibevoice_hip_diag.h")):
    names = set()
    for h in headers:
        src = open(os.path.join(ROOT, "include", h)).read()
        names |= set(re.findall(r"^\s*(?:const char\*|int|void)\s+(vv_\w+)\(", src, re.M))
    return sorted(names)


def test_header_declares_entry_points():
    names = declared_symbols()
    assert "vv_lm_forward" in names and "vv_diffusion_sample" in names and "vv_codec_step" in names
    assert set(names) == {n for n, _, _ in _lib.EXPORTS}


def test_product_header_has_no_diagnostics():
    """Tuning hooks, stamps, kernel entry points and benchmark-only switches
    (process-wide state) live in the diag header only."""
    product = set(declared_symbols(("vibevoice_hip.h",)))
    diag = set(declared_symbols(("vibevoice_hip_diag.h",)))
    assert not product & diag
    for n in product:
        assert not re.search(r"tune|stamps|null_collective|synthetic|_bf16$|plan|chain|pack|rope_table|defer|"
                             r"mix_fusion|attn_prefill", n), n
    assert {"vv_tp_null_collective", "vv_kv_synthetic", "vv_gemv_tune", "vv_gemm_bf16"} <= diag
    # nothing in the product package calls a diagnostic entry point
    pkg = os.path.join(ROOT, "vibevoice_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py") and f != "_lib.py":
            src = open(os.path.join(pkg, f)).read()
            for n in diag:
                assert n + "(" not in src, (f, n)


def test_library_loads_and_exports_all_symbols():
    L = _lib.lib()
    for name in declared_symbols():
        assert hasattr(L, name), name


def test_config_struct_matches_header():
    # vv_config: 6 ints, 2 floats, 3 ints, 1 float, 1 int, 3 x int[8], 4 ints, 1 float, 2 ints
    assert ctypes.sizeof(_lib.VVConfig) == 4 * (6 + 2 + 3 + 1 + 1 + 24 + 4 + 1 + 2)


def test_create_rejects_bad_config():
    L = _lib.lib()
    c = _lib.VVConfig()
    c.head_dim = 64
    h = ctypes.c_void_p()
    assert L.vv_create(ctypes.byref(c), 0, ctypes.byref(h)) != 0
    assert b"head_dim" in L.vv_last_error()


def _plan(M, N, K, xf=0, w=False, mod=False):
    out = (ctypes.c_int * 7)()
    assert _lib.lib().vv_gemv_plan(M, N, K, xf, int(w), int(mod), out) == 0
    return dict(zip(("kernel", "waves", "ksplit", "u", "tpw", "rw", "lds"), list(out)))


def test_gemv_plan_rules():
    """The decode-GEMV launch plans DESIGN.md §3 documents (host logic only)."""
    NORM = 1
    # B = 1 (M = 2): LM gate|up, 2-wave one-tile workgroups, row-per-wave norm
    p = _plan(2, 17920, 1536, NORM, w=True)
    assert (p["kernel"], p["waves"], p["ksplit"], p["u"], p["tpw"], p["rw"]) == (0, 2, 1, 4, 1, 1)
    # B = 8 (M = 16): 8 tiles per 8-wave workgroup, two rows per wave
    p = _plan(16, 17920, 1536, NORM, w=True)
    assert (p["waves"], p["tpw"], p["rw"]) == (8, 8, 1)
    # B = 8 LM down: K split until the A slice fits 64 KB of LDS (5 ways), staged once
    p = _plan(16, 1536, 8960)
    assert (p["kernel"], p["ksplit"], p["waves"]) == (0, 5, 8) and p["lds"] <= 65536
    # codec fc1 at C = 2,048 (512 tiles), B = 8: two tiles per workgroup (256 workgroups)
    p = _plan(8, 8192, 2048)
    assert (p["kernel"], p["tpw"], p["waves"]) == (0, 2, 8)
    # codec fc2 at C = 2,048 keeps its 2-way split on k_gemv (the split-to-fit rule cost 20 us there)
    p = _plan(16, 2048, 8192)
    assert (p["kernel"], p["ksplit"], p["waves"]) == (1, 2, 8)
    # VibeVoice-Large LM down at M = 2: split until the 76 KB of A rows fit
    p = _plan(2, 3584, 18944)
    assert (p["kernel"], p["ksplit"], p["waves"]) == (0, 2, 8)
    # Large head layers (K 3,584, norm weight + adaLN): the LDS-DMA row form; no adaLN: registers
    assert _plan(2, 21504, 3584, NORM, w=True, mod=True)["rw"] == 2
    assert _plan(2, 37888, 3584, NORM, w=True)["rw"] == 1
    # the RW form is an XF_NORM-only, unsplit-K form
    assert _plan(2, 1536, 8960)["rw"] == 0
    assert _plan(16, 64, 1536, NORM, mod=True)["ksplit"] == 8 and _plan(16, 64, 1536, NORM, mod=True)["rw"] == 0
    # the diagnostic switch turns it off and back on
    L = _lib.lib()
    L.vv_gemv_tune_rw(99)
    try:
        assert _plan(2, 17920, 1536, NORM, w=True)["rw"] == 0
    finally:
        L.vv_gemv_tune_rw(0)
    assert _plan(2, 17920, 1536, NORM, w=True)["rw"] == 1


KINDS = ("GEMV1", "GEMV", "GEMVW", "GEMV_W8", "GEMM64", "GEMM32", "GEMM_BIG1", "GEMM_BIG2", "GEMM_XL", "REJECT")


def _gemm(M, N, K, xf=0, w=False, mod=False, epi=0, keep=0, cus=256):
    out = (ctypes.c_int * 11)()
    assert _lib.lib().vv_gemm_plan(M, N, K, xf, int(w), int(mod), epi, keep, cus, out, 11) == 0
    p = dict(zip(("kind", "mrep", "waves", "ksplit", "u", "tpw", "rw", "grid_x", "grid_y", "block", "lds"), list(out)))
    p["kind"] = KINDS[p["kind"]]
    return p


# test_gpu_gemm.py's test_tiled_store and test_gemm_big_tile shapes, and 16K-row prefill projections
TILED = [(M, N, K) for M in (65, 200, 3200) for N, K in ((128, 32), (32, 128), (512, 128), (64, 256), (2048, 1536))] + [
    (256, 2048, 1536), (257, 1536, 1536), (1000, 1536, 8960), (1000, 17920, 1536), (4100, 2048, 1536), (300, 1024, 512),
    (640, 512, 128), (16384, 2048, 1536), (16384, 1536, 8960), (16384, 17920, 1536)]


def test_gemm_launch_decision():
    """The one launch decision (csrc/gemm.hip gemm_decide, read by launch_gemm)
    where vv_gemv_plan cannot look: the CU-count-dependent balanced form, the
    M > 16 kernels and the tiled ladder (host logic only)."""
    L = _lib.lib()
    NORM, EPI_CFG_DPM = 1, 6
    assert L.vv_gemm_plan(16, 64, 64, 0, 0, 0, 0, 0, 256, (ctypes.c_int * 10)(), 10) != 0      # out[] too short
    # balanced many-tile form: B = 8 LM gate|up, 1,120 tiles on 256 CUs = 5 tiles per workgroup, 2 waves each
    p = _gemm(16, 17920, 1536, NORM, w=True, cus=256)
    assert (p["kind"], p["tpw"], p["waves"], p["grid_x"], p["grid_y"]) == ("GEMV1", 5, 10, 256, 1)
    p = _gemm(16, 17920, 1536, NORM, w=True, cus=0)
    assert (p["kind"], p["tpw"], p["waves"], p["grid_x"]) == ("GEMV1", 8, 8, 140)
    L.vv_gemv_tune_bal(0)
    try:
        p = _gemm(16, 17920, 1536, NORM, w=True, cus=256)
        assert (p["kind"], p["tpw"], p["waves"], p["grid_x"]) == ("GEMV1", 8, 8, 140)
    finally:
        L.vv_gemv_tune_bal(1)
    # 16 < M <= 64 with >= 256 tiles: k_gemvw, 4 tiles per 8-wave workgroup at >= 1,024 tiles
    p = _gemm(32, 17920, 1536)
    assert (p["kind"], p["mrep"], p["tpw"], p["grid_x"], p["block"]) == ("GEMVW", 2, 4, 280, 512)
    L.vv_gemv_tune_wide(0)
    try:
        p = _gemm(32, 17920, 1536)
        assert (p["kind"], p["mrep"]) == ("GEMV", 2)
    finally:
        L.vv_gemv_tune_wide(1)
    # the tiled ladder, one shape per rung: 256² tile, 128² tile (2 / 1 LDS stages), 64- and 32-wide k_gemm
    p = _gemm(16384, 2048, 1536)
    assert (p["kind"], p["grid_x"], p["grid_y"], p["block"], p["lds"]) == ("GEMM_XL", 64 * 8, 1, 512, 128 * 1024)
    p = _gemm(3200, 2048, 1536)          # 13 x 8 = 104 256² tiles (< 192), 25 x 16 = 400 128² tiles (>= 256)
    assert (p["kind"], p["grid_x"], p["block"]) == ("GEMM_BIG2", 400, 256)
    p = _gemm(200, 2048, 1536)           # < 256 rows: 4 x 32 = 128 64-wide workgroups
    assert (p["kind"], p["grid_x"], p["grid_y"]) == ("GEMM64", 4, 32)
    p = _gemm(200, 512, 128)             # 4 x 8 = 32 such workgroups (< 128): 32-wide tiles
    assert (p["kind"], p["grid_x"], p["grid_y"]) == ("GEMM32", 4, 16)
    assert _gemm(300, 1024, 512)["kind"] == "GEMM32"      # 24 128² tiles, < 2^30 MACs: stays on k_gemm
    for mode, kinds in ((0, ("GEMM64", "GEMM64", "GEMM32")), (1, ("GEMM_BIG1", "GEMM_BIG1", "GEMM32")),
                        (2, ("GEMM_BIG2", "GEMM_BIG2", "GEMM32")), (-1, ("GEMM_XL", "GEMM_BIG2", "GEMM32")),
                        (5, ("GEMM_BIG1", "GEMM_BIG1", "GEMM_BIG1")), (7, ("GEMM_XL", "GEMM_XL", "GEMM_XL"))):
        L.vv_gemm_tune_big(mode)
        try:
            got = tuple(_gemm(*s)["kind"] for s in ((16384, 2048, 1536), (3200, 2048, 1536), (300, 1024, 512)))
        finally:
            L.vv_gemm_tune_big(-1)
        assert got == kinds, (mode, got)
    # gemm_uses_xl (the A-row layout engine.cpp's producers write) = "the decision is GEMM_XL": mode 3 (-1) of
    # vv_gemm_tune_big, >= 256 rows, N % 256 == 0, K % 32 == 0 and >= 192 such tiles, or any count with + 4
    for mode in (-1, 0, 1, 2, 4, 5, 6, 7):
        L.vv_gemm_tune_big(mode)
        try:
            got = [_gemm(*s)["kind"] == "GEMM_XL" for s in TILED]
        finally:
            L.vv_gemm_tune_big(-1)
        big, any_count = (3, 0) if mode < 0 else (mode & 3, mode & 4)
        want = [big == 3 and M >= 256 and N % 256 == 0 and K % 32 == 0 and (-(-M // 256) * (N // 256) >= 192 or
                                                                           bool(any_count)) for M, N, K in TILED]
        assert got == want, mode
    assert any(want) and not all(want)
    # an A transform keeps the prefill shape off the LDS-staged tiles
    assert _gemm(16384, 2048, 1536, NORM, w=True)["kind"] == "GEMM64"
    # no kernel: N % 32 != 0 on the tiled path, the CFG + DPM epilogue at more than 16 rows
    assert _gemm(128, 48, 64)["kind"] == "REJECT" and _gemm(64, 48, 64)["kind"] == "GEMV"
    assert _gemm(18, 64, 1536, NORM, epi=EPI_CFG_DPM)["kind"] == "REJECT"
    assert _gemm(16, 64, 1536, NORM, epi=EPI_CFG_DPM)["kind"] == "GEMV1"


def _attn(ntok, max_pos_p1, lm_slots=2):
    out = (ctypes.c_int * 6)()
    assert _lib.lib().vv_attn_pass_plan(ntok, lm_slots, 128, 2, max_pos_p1, out) == 0
    return dict(zip(("prefill", "nsplit", "chunk", "defer", "group", "ngroups"), list(out)))


def test_attention_pass_plan_rules():
    """The decode attention plans DESIGN.md §3 documents (host logic only)."""
    L = _lib.lib()
    # B = 1 short context: 2..8 deferred splits of >= 128 keys, merged by o_proj
    p = _attn(2, 900)
    assert (p["prefill"], p["defer"], p["nsplit"], p["chunk"], p["group"]) == (0, 1, 8, 128, 0)
    # B = 8 (16 rows) does not defer: one 1,024-key split per (row, kv head) at this length
    p = _attn(16, 900, lm_slots=16)
    assert (p["defer"], p["nsplit"], p["group"]) == (0, 1, 0)
    # 64K: at most 120 splits of >= 256 keys in <= 8 groups of <= 16 (one CU per keyed workgroup)
    p = _attn(2, 65040)
    assert (p["nsplit"], p["chunk"], p["group"], p["ngroups"]) == (120, 544, 15, 8)
    p = _attn(2, 20000)
    assert (p["nsplit"], p["chunk"], p["group"], p["ngroups"]) == (79, 256, 10, 8)
    # the switch: 0 = 1,024-key splits merged by k_attn_merge; n = at most n splits
    L.vv_attn_group(0)
    try:
        p = _attn(2, 65040)
        assert (p["nsplit"], p["chunk"], p["group"]) == (64, 1024, 0)
        L.vv_attn_group(128)
        assert _attn(2, 65040)["nsplit"] == 128
    finally:
        L.vv_attn_group(1)
    assert _attn(2, 65040)["nsplit"] == 120
    # the kernels' limits, over every context the group plan takes: k_attn's group
    # merge holds <= 16 split partials, o_proj's XF_ATTN_MERGE <= 8 group partials
    for max_len in range(8193, 65537, 997):
        p = _attn(2, max_len)
        if p["group"]:
            assert p["group"] <= 16 and p["ngroups"] <= 8 and p["nsplit"] <= 128
            assert p["ngroups"] * p["group"] * p["chunk"] >= max_len
    # grouped merge, ragged rows in one pass (the plan is sized by the longest row):
    # the producer's active groups for a row of n keys, ceil(ceil(n / chunk) / group),
    # equal the consumer's ceil(n / (group * chunk)) and never exceed ngroups
    for max_len in (8193, 20000, 32768, 65040, 65536):
        p = _attn(2, max_len)
        ch, gs, ng = p["chunk"], p["group"], p["ngroups"]
        assert gs > 0 and ng * gs * ch >= max_len
        for n in (1, 200, ch - 1, ch, ch + 1, gs * ch, gs * ch + 1, max_len // 3, max_len - 1, max_len):
            prod = -(-(-(-n // ch)) // gs)
            cons = min(-(-n // (gs * ch)), ng)
            assert prod == cons <= ng, (max_len, n, prod, cons)
    # a prompt: the prefill kernel (>= 256 rows and >= 32 rows per slot), no splits
    p = _attn(512, 512)
    assert (p["prefill"], p["nsplit"]) == (1, 1)


def test_attention_row_splits():
    """The per-row key-split plan that k_attn, k_attn_merge, k_attn_finish and o_proj's XF_ATTN_MERGE all
    evaluate (attn_dev.h attn_row_splits, through vv_diag_attn_row_splits): the row's split size is a
    multiple of 32 and at least the launch's, its active splits cover the row with none to spare, and the
    grouped count is ceil(active / group) -- equal to the rule stated here in plain Python."""
    f = _lib.lib().vv_diag_attn_row_splits
    out = (ctypes.c_int * 3)()
    lens = list(range(1, 2101)) + [4095, 4096, 4097, 65535, 65536]
    for nsplit, chunk in ((1, 1024), (8, 32), (8, 64), (64, 1024), (256, 1024)):
        for group in (0, 2, 16):
            for n in lens:
                assert f(n, nsplit, chunk, group, out) == 0
                ch, nact, nparts = out[0], out[1], out[2]
                assert ch % 32 == 0 and ch >= chunk, (n, nsplit, chunk, ch)
                assert 1 <= nact <= nsplit, (n, nsplit, chunk, nact)
                assert nact * ch >= n > (nact - 1) * ch, (n, nsplit, chunk, ch, nact)
                want_ch = max(chunk, -(-(-(-n // nsplit)) // 32) * 32)
                want_nact = -(-n // want_ch)
                want_parts = -(-want_nact // group) if group else want_nact
                assert (ch, nact, nparts) == (want_ch, want_nact, want_parts), (n, nsplit, chunk, group)
    assert f(0, 8, 32, 0, out) != 0 and f(1, 0, 32, 0, out) != 0 and f(1, 257, 32, 0, out) != 0
    assert f(1, 8, 48, 0, out) != 0 and f(1, 8, 0, 0, out) != 0 and f(1, 8, 32, -1, out) != 0
    assert f(1, 8, 32, 0, None) != 0


def test_persist_decision_rule():
    """The rule every grid-waiting launch applies before it is issued (VERDICT
    r5 item 8; host logic only): the whole one-per-CU grid resident by the
    occupancy query, no scratch, the kernels enabled for the context, and the
    context the device's only registered one -- else the GEMV launches run."""
    d = _lib.lib().vv_persist_decision
    assert d(1, 256, 0, 256, 1, 1) == 1
    assert d(2, 256, 0, 256, 1, 1) == 1          # more room than needed
    assert d(1, 240, 0, 256, 1, 1) == 0          # fewer CUs (e.g. a CU mask) than workgroups
    assert d(0, 256, 0, 256, 1, 1) == 0          # the build does not fit a CU
    assert d(1, 256, 64, 256, 1, 1) == 0         # scratch: waves may wait for slots
    assert d(1, 256, 0, 256, 2, 1) == 0          # a second registered context on the device
    assert d(1, 256, 0, 256, 1, 0) == 0          # switched off (VIBEVOICE_PERSISTENT=0 / vv_set_persistent)


def test_lm_attn_form_table():
    """k_lm_attn's seven built forms (lm_attn.hip la_form: the table the launcher looks up): FP8 weights x KV
    form x short / long.  kvq = 2 (the diagnostic) is built for bf16 weights only and the kvq forms at no more
    than 4,096 keys: those five combinations, and keys outside 1 .. 2^20, are refused."""
    f = _lib.lib().vv_diag_lm_attn_form
    out = (ctypes.c_int * 3)()
    built = set()
    for w8 in (0, 1):
        for kvq in (0, 1, 2):
            for keys in (1, 4096, 4097, 1 << 20):
                lng = int(keys > 4096)
                exists = not (kvq == 2 and w8) and not (kvq != 0 and lng)
                out[0] = out[1] = out[2] = -1
                rc = f(w8, kvq, keys, out)
                assert (rc == 0) == exists, (w8, kvq, keys, rc)
                if exists:
                    assert tuple(out) == (w8, kvq, lng), (w8, kvq, keys, tuple(out))
                    built.add(tuple(out))
                else:
                    assert tuple(out) == (-1, -1, -1)
                assert f(w8, kvq, 0, out) != 0 and f(w8, kvq, (1 << 20) + 1, out) != 0
    assert built == {(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 2, 0), (0, 0, 1), (1, 0, 1)}
    assert sum(f(w8, kvq, keys, out) != 0 for w8 in (0, 1) for kvq in (0, 1, 2) for keys in (4096, 4097)) == 5
    assert f(0, 0, 1, None) != 0 and f(2, 0, 1, out) != 0 and f(0, 3, 1, out) != 0 and f(0, -1, 1, out) != 0
