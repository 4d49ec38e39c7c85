"""The grid-wait counters between two launches (vv_diag_sync_words; the layout is
vibevoice_amd/csrc/sync_layout.h).  Kernels that wait on the same buffer share
its shard lines, which is sound only while every launch leaves every counter at
a whole number of waits -- after a clean run, and after vv_sync_reset."""
import ctypes

from vibevoice_amd import _lib

LINES = 16                    # counter lines per buffer; then one ticket-residue word
SHARD_LINES = range(8)        # 32 arrivals per shard per wait
GEN_LINES = (11, 12, 15)      # 8 bumps per wait
N_WORDS = 3 * (LINES + 1) + 2


def assert_counters_consistent(eng):
    """Every shard line a multiple of 32 arrivals, every generation line a
    multiple of 8, every k_lm_ffn16 ticket a multiple of 4 (the buffer's highest
    ticket % 4 is 0), every wide-stage cluster counter a multiple of its cluster
    size (highest residue 0 for C = 256 and for C = 512).  The raise hook leaves
    shard 0 at +5, the generations at +3, a ticket at +1 and a cluster counter of
    each C at +3, as a launch that gave up does; only vv_sync_reset makes them
    consistent again."""
    words = (ctypes.c_uint * N_WORDS)()
    _lib.check(_lib.lib().vv_diag_sync_words(eng.h, words, N_WORDS), "sync_words")
    for fam in range(3):      # head, codec stage, LM
        w = list(words[fam * (LINES + 1):(fam + 1) * (LINES + 1)])
        assert all(w[i] % 32 == 0 for i in SHARD_LINES), (fam, w)
        assert all(w[i] % 8 == 0 for i in GEN_LINES), (fam, w)
        assert w[LINES] == 0, (fam, w)
    assert list(words[3 * (LINES + 1):]) == [0, 0], list(words)
