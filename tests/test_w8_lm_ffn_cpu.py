"""The switch of the one-launch LM MLP kernels' W8 forms (host only, no device
work): vv_lm_ffn_w8 is exported, bound by _lib.py, accepts the bit sets 0..3
(bit 0: <= 2 rows, bit 1: 3..16 rows) and rejects everything else, and every
accepted call bumps the workspace epoch so hosts drop graphs that captured the
other path."""
import re
from pathlib import Path

from vibevoice_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def test_symbol_is_exported_and_bound():
    L = _lib.lib()   # raises if the library does not load
    fn = L.vv_lm_ffn_w8
    assert fn.argtypes is not None and len(fn.argtypes) == 1
    header = (ROOT / "include" / "vibevoice_hip_diag.h").read_text()
    assert re.search(r"^int vv_lm_ffn_w8\(int bits\);", header, re.M)


def test_accepts_the_four_bit_sets_and_rejects_others():
    L = _lib.lib()
    try:
        for bits in (0, 1, 2, 3):
            e0 = L.vv_ws_epoch()
            assert L.vv_lm_ffn_w8(bits) == 0, bits
            assert L.vv_ws_epoch() != e0, bits
        for bad in (-1, 4, 7, 256):
            e0 = L.vv_ws_epoch()
            assert L.vv_lm_ffn_w8(bad) != 0, bad
            assert b"vv_lm_ffn_w8" in L.vv_last_error()
            assert L.vv_ws_epoch() == e0, bad
    finally:
        assert L.vv_lm_ffn_w8(3) == 0
