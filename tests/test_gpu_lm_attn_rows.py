"""The one-launch LM attention kernel at 17 to 32 rows (lm_attn.hip: k_lm_attn's second row
class, MT = 2; the per-engine option lm_attn_max_rows / vv_set_lm_attn_max_rows, default 16).

Every value of a row depends only on that row's A row, the weights and its own KV entries, and
per row the second row class runs the first one's arithmetic in the first one's order.  So a
pass of 17 .. 32 rows must give, row by row, the bits the same rows give in passes of at most 16
rows on the same KV state: an engine with the option runs one R-row pass, an engine without it
runs the rows as passes of at most 16 (the 16-row class), and everything is compared with
torch.equal -- no tolerance, and not the code against itself.  The oracle and the three launches
bound the R = 32 pass as test_gpu_lm.py bounds the 16-row kernel (rel L2 < 2e-2, cosine > 0.999).

Engines have the 1.5B layer shapes (H 1536, 12 / 2 heads of 128, I 8960) and are built one after
another: a one-launch kernel runs only while its context is the device's only registered one.
"""
import ctypes
import gc

import pytest
import torch

from gpu_util import cos, rel_err
from oracle import lm as olm
from sync_counters import assert_counters_consistent
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
dev = "cuda"
I32 = dict(dtype=torch.int32, device=dev)
BF = dict(dtype=torch.bfloat16, device=dev)
VALID = [151643, 151652, 151653, 151654]
FP8 = "fp8_e4m3"
H, I, NH, NKV, HD = 1536, 8960, 12, 2, 128
LMP = "model.language_model."
STEPS = 3
# ragged row lengths, 1 .. ~600 keys: both sides of the 32-key unit edges (1, 31, 32, 33, 64), rows of one
# unit and of many; row 16 -- the one row of the second tile at R = 17 -- has 33 keys, row 30 has 1
LENS = (1, 31, 32, 33, 64, 200, 597, 2, 95, 128, 17, 333, 63, 65, 400, 7,
        33, 160, 96, 3, 250, 30, 34, 129, 580, 12, 48, 72, 301, 5, 1, 223)


@pytest.fixture(autouse=True)
def _switches():
    gc.collect()
    yield
    _lib.lib().vv_lm_attn(1)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _cfg():
    return tiny_config(hidden=H, layers=2, heads=NH, kv_heads=NKV, inter=I)


def _sd(cfg, seed):
    return synthetic_state_dict(cfg, seed=seed, device="cpu", mode="test", with_acoustic_encoder=False)


def _engine(cfg, sd, max_batch, max_ctx, **kw):
    return Engine(cfg, sd, dev, max_batch=max_batch, max_ctx=max_ctx, valid_ids=VALID, **kw)


def _close(eng):
    eng.close()
    del eng
    gc.collect()


def oracle_sd(sd):
    return {k[len(LMP):]: v for k, v in sd.items() if k.startswith(LMP)}


def _spread_exponents(cfg, sd):
    """Row n of every layer's v_proj and o_proj times 2^((n mod 13) - 6), q_proj and k_proj rows times
    2^((n mod 3) - 1): the rows of one 16-row weight tile get exponents over several binades
    (tests/test_gpu_w8_lm_attn.py's weights)."""
    def scaled(w, e):
        return torch.ldexp(w.float(), e[:, None].to(torch.int32)).to(w.dtype)
    for l in range(cfg.decoder_config.num_hidden_layers):
        p = f"{LMP}layers.{l}.self_attn."
        for n, (m, o) in zip("qkvo", ((3, 1), (3, 1), (13, 6), (13, 6))):
            w = sd[p + n + "_proj.weight"]
            sd[p + n + "_proj.weight"] = scaled(w, torch.arange(w.shape[0]) % m - o)
    return sd


def _chunks(R):
    """The rows of an R-row pass as passes of at most 16 rows."""
    return [(a, min(a + 16, R)) for a in range(0, R, 16)]


def _pass(eng, x, rows, pos, max_pos, active, halves=False):
    """One decode pass of the rows [a, b) of the case (row r sits in slot r); hidden bits, logits, and the pass's
    q rows (last layer) and appended K / V rows of both layers, read through vv_diag_lm_qkv.  halves: the
    layers' attention halves alone (vv_lm_attn_replay: layer 1 reads x + layer 0's attention half, no MLP, no
    head), so only the q / K / V rows."""
    L = _lib.lib()
    a, b = rows
    n = b - a
    sl, pp, xx = torch.arange(a, b).to(**I32), pos[a:b].to(**I32), x[a:b].contiguous()
    assert L.vv_lm_attn_active(eng.h, n, max_pos + 1) == active, (n, max_pos, active)
    if halves:
        _lib.check(L.vv_lm_attn_replay(eng.h, n, P(xx), P(sl), P(pp), max_pos + 1, 1, None), "lm_attn_replay")
        torch.cuda.synchronize()
        out = []
    else:
        h, lg = eng.lm_forward(xx, sl, pp, torch.arange(n).to(**I32), max_pos=max_pos)
        torch.cuda.synchronize()
        out = [bits(h), lg.cpu()]
    ar = (ctypes.c_int * n)(*range(a, b))
    pp = (ctypes.c_int * n)(*pos[a:b].tolist())
    for l in range(2):
        q, k, v = torch.empty(n, NH * HD, **BF), torch.empty(n, NKV, HD, **BF), torch.empty(n, NKV, HD, **BF)
        _lib.check(L.vv_diag_lm_qkv(eng.h, n, l, ar, pp, P(q), P(k), P(v)), "diag_lm_qkv")
        out += [bits(q), bits(k), bits(v)]
    return out


def _decode(eng, xs, lens, passes, max_pos, active, halves=False):
    """STEPS decode steps over the rows, each step as the given passes; per step the passes' results joined."""
    res = []
    for s in range(STEPS):
        pos = torch.tensor(lens) + s
        parts = [_pass(eng, xs[s], rows, pos, max_pos, act, halves) for rows, act in zip(passes, active)]
        res.append([torch.cat(t) for t in zip(*parts)])
    eng.check_sync()
    assert_counters_consistent(eng)
    return res


def _prefill(eng, xp, lens):
    slots = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(n) for n in lens]).to(**I32)
    last = (torch.cumsum(torch.tensor(lens), 0) - 1).to(**I32)
    eng.lm_forward(xp, slots, pos, last)
    torch.cuda.synchronize()


NAMES = ("hidden", "logits", "q", "k0", "v0", "q", "k1", "v1")


def _assert_equal(ra, rb, tag):
    """Every figure printed first, then asserted."""
    for s, (a, b) in enumerate(zip(ra, rb)):
        names = NAMES[-len(a):]
        diff = {n: f"{int((x != y).sum())} of {x.numel()}" for n, x, y in zip(names, a, b)}
        print(f"{tag} step {s}: values that differ: {diff}")
    for s, (a, b) in enumerate(zip(ra, rb)):
        names = NAMES[-len(a):]
        assert all(torch.isfinite(t.view(torch.bfloat16).float()).all() and t.any() for t in a[-6:])
        for n, x, y in zip(names, a, b):
            assert torch.equal(x, y), (tag, s, n)


# ------------------------------------------------------------------ 1. bitwise against the 16-row kernel
@pytest.mark.parametrize("halves", [True, False], ids=["attention_halves", "whole_pass"])
@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("R", [16, 17, 24, 31, 32])
def test_rows_compute_the_16_row_kernels_bits(R, w8, halves):
    """Engine A (lm_attn_max_rows = 32) runs one R-row pass per step, engine B (no option) the same rows as
    passes of at most 16; at R = 16 both run the 16-row class.

    attention_halves: both layers' attention halves alone (vv_lm_attn_replay) -- k_lm_attn and nothing else;
    layer 1's q / K / V rows are functions of layer 0's whole attention half.

    whole_pass: the hidden rows and logits of vv_lm_forward too.  The GEMMs of 17 .. 32 rows sum K in another
    order than the kernels of 16 rows or fewer (with the one-launch kernel off on both engines 4,597 of 26,112
    hidden values differ at R = 17), so a pass that ran the second row class runs its MLP as the passes of at most
    16 rows it is made of (engine.cpp lm_mlp_half); without that 2,271 hidden values differ at R = 17, bf16."""
    L = _lib.lib()
    cfg = _cfg()
    sd = _sd(cfg, 131)
    kw = {}
    if w8:
        sd, kw = _spread_exponents(cfg, sd), dict(weight_dtype=FP8, lm_attn_w8=True)
    lens = list(LENS[:R])
    g = torch.Generator().manual_seed(132 + R)
    xp = torch.randn(sum(lens), H, generator=g).bfloat16().to(dev)
    xs = [torch.randn(R, H, generator=g).bfloat16().to(dev) for _ in range(STEPS)]
    mp = max(lens) + STEPS
    a = _engine(cfg, sd, 16, 1024, lm_attn_max_rows=32, **kw)
    assert L.vv_lm_attn_max_rows(a.h) == 32 and a.lm_attn_max_rows == 32 and a.weights_quantized() == w8
    _prefill(a, xp, lens)
    ra = _decode(a, xs, lens, [(0, R)], mp, [1], halves)
    _close(a)
    b = _engine(cfg, sd, 16, 1024, **kw)
    assert L.vv_lm_attn_max_rows(b.h) == 16 and b.lm_attn_max_rows is None
    assert L.vv_lm_attn_active(b.h, R, mp + 1) == (1 if R <= 16 else 0)
    _prefill(b, xp, lens)
    rb = _decode(b, xs, lens, _chunks(R), mp, [1] * len(_chunks(R)), halves)
    _close(b)
    _assert_equal(ra, rb, f"R={R} {'w8' if w8 else 'bf16'} {'attention halves' if halves else 'whole pass'}")


# ------------------------------------------------------------------ 2. against the oracle and the three launches
def test_32_rows_vs_oracle_and_three_launches():
    L = _lib.lib()
    R = 32
    cfg = _cfg()
    sd = _sd(cfg, 133)
    lcfg, osd = dict(cfg.decoder_config), oracle_sd(sd)
    lens = [min(n, 70) for n in LENS]   # (the oracle prefills on the CPU: 1 .. 70 keys, the same unit edges)
    g = torch.Generator().manual_seed(134)
    xr = [torch.randn(n, H, generator=g).bfloat16() for n in lens]
    kvs = [olm.RowKV(2) for _ in lens]
    for r in range(R):
        olm.forward_rows(osd, lcfg, xr[r][None], kvs[r:r + 1])
    eng = _engine(cfg, sd, 16, 1024, lm_attn_max_rows=32)
    _prefill(eng, torch.cat(xr).to(dev), lens)
    ar = torch.arange(R).to(**I32)
    try:
        for s in range(STEPS):
            x = torch.randn(R, H, generator=g).bfloat16()
            ref = olm.forward_rows(osd, lcfg, x[:, None], kvs)[:, -1]
            pos = (torch.tensor(lens) + s).to(**I32)
            outs = {}
            for on in (0, 1, 1, 15):   # 15: every issue-order variant bit cleared
                L.vv_lm_attn(on)
                assert L.vv_lm_attn_active(eng.h, R, max(lens) + s + 1) == (1 if on else 0)
                h, lg = eng.lm_forward(x.to(dev), ar, pos, ar)
                torch.cuda.synchronize()
                outs.setdefault(on, []).append((h.clone(), lg.clone()))
            (one, lg1), (three, _) = outs[1][0], outs[0][0]
            for r in range(R):
                e_o, c_o, e_3, c_3 = rel_err(one[r], ref[r]), cos(one[r], ref[r]), rel_err(one[r], three[r]), cos(one[r], three[r])
                print(f"step {s} row {r} len {lens[r] + s + 1}: oracle rel {e_o:.2e} cos {c_o:.5f}; three launches rel {e_3:.2e} cos {c_3:.5f}")
                assert e_o < 2e-2 and c_o > 0.999 and e_3 < 2e-2 and c_3 > 0.999, (s, r)
            for h, lg in (outs[1][1], outs[15][0]):   # a repeat run and the issue-order variant: the same sums
                assert torch.equal(bits(one), bits(h)) and torch.equal(lg1, lg)
    finally:
        L.vv_lm_attn(1)
    eng.check_sync()
    assert_counters_consistent(eng)
    _close(eng)


# ------------------------------------------------------------------ 3. the long form
LONG_ROWS = {3: 4096, 19: 8187}   # row index -> cached keys: 4,097 (s = 2) and 8,188 keys at the first step


@pytest.mark.parametrize("halves", [True, False], ids=["attention_halves", "whole_pass"])
def test_long_form_20_rows(halves):
    """20 rows planned at 8,191 keys: 18 short rows (2 .. 200 keys, s = 1) and two long ones, one in each row tile,
    so units of one and of two steps share a pass.  Against passes of at most 16 rows (the long form of the 16-row
    class) on an engine with lm_attn_max_keys only; the two modes of test_rows_compute_the_16_row_kernels_bits."""
    L = _lib.lib()
    R = 20
    cfg = _cfg()
    sd = _sd(cfg, 135)
    g = torch.Generator().manual_seed(136)
    lens = [LONG_ROWS.get(r, 1 + (r * 53) % 199) for r in range(R)]   # cached keys; + 1 = the row's keys at step 0
    assert all(2 <= n + 1 <= 200 for r, n in enumerate(lens) if r not in LONG_ROWS)
    rows = [(torch.randn(2, NKV, n, HD, generator=g).bfloat16(), torch.randn(2, NKV, n, HD, generator=g).bfloat16())
            for n in lens]
    xs = [torch.randn(R, H, generator=g).bfloat16().to(dev) for _ in range(STEPS)]

    def run(eng, passes):
        for r, (k, v) in enumerate(rows):
            k, v = k.to(dev).contiguous(), v.to(dev).contiguous()
            _lib.check(L.vv_diag_kv_write(eng.h, r, 0, lens[r], P(k), P(v)), "diag_kv_write")
        torch.cuda.synchronize()
        return _decode(eng, xs, lens, passes, 8190, [1] * len(passes), halves)

    a = _engine(cfg, sd, 10, 8192, lm_attn_max_keys=8191, lm_attn_max_rows=32)
    ra = run(a, [(0, R)])
    _close(a)
    b = _engine(cfg, sd, 10, 8192, lm_attn_max_keys=8191)
    assert L.vv_lm_attn_active(b.h, R, 8191) == 0
    rb = run(b, _chunks(R))
    _close(b)
    _assert_equal(ra, rb, f"long form, 20 rows, {'attention halves' if halves else 'whole pass'}")


# ------------------------------------------------------------------ 4. the option's errors
def test_option_errors():
    L = _lib.lib()
    cfg = _cfg()
    sd = _sd(cfg, 137)
    a = _engine(cfg, sd, 16, 256, lm_attn_max_rows=24)
    assert L.vv_lm_attn_max_rows(a.h) == 24
    assert [L.vv_lm_attn_active(a.h, r, 64) for r in (16, 17, 24, 25, 32)] == [1, 1, 1, 0, 0]
    assert L.vv_set_lm_attn_max_rows(a.h, 32) != 0 and b"vv_set_lm_attn_max_rows after vv_finalize" in L.vv_last_error()
    assert L.vv_lm_attn_max_rows(a.h) == 24
    L.vv_lm_attn(0)
    assert L.vv_lm_attn_active(a.h, 17, 64) == 0
    L.vv_lm_attn(1)
    _close(a)
    for bad in (15, 33):
        with pytest.raises(ValueError, match="outside"):
            _engine(cfg, sd, 16, 256, lm_attn_max_rows=bad)
    with pytest.raises(ValueError, match="tensor parallelism"):
        Engine(cfg, sd, dev, max_batch=16, max_ctx=256, tp_size=2, lm_attn_max_rows=32)
    # the C entry point's own range check: a context that is created and not finalized
    h = ctypes.c_void_p()
    from vibevoice_amd.engine import engine_config
    ecfg = engine_config(cfg, 16, 256, 1, False)
    _lib.check(L.vv_create(ctypes.byref(ecfg), 0, ctypes.byref(h)), "create")
    try:
        for bad in (15, 33, 0, -1):
            assert L.vv_set_lm_attn_max_rows(h, bad) != 0 and b"is outside [16, 32]" in L.vv_last_error()
        assert L.vv_lm_attn_max_rows(h) == 16
        assert L.vv_set_lm_attn_max_rows(h, 32) == 0 and L.vv_lm_attn_max_rows(h) == 32
    finally:
        L.vv_destroy(h)
    # no FP8-KV form is built above 16 rows: such an engine keeps its launches there
    f = _engine(cfg, sd, 16, 256, kv_dtype=FP8, lm_attn_kv8=True, lm_attn_max_rows=32)
    assert L.vv_lm_attn_max_rows(f.h) == 32
    assert L.vv_lm_attn_active(f.h, 16, 64) == 1 and L.vv_lm_attn_active(f.h, 17, 64) == 0
    _close(f)


# ------------------------------------------------------------------ 5. generate() end to end
def test_generate_9_dialogues():
    """B = 9: 18 decode rows.  With the option, eager and graph replay give the same tokens and audio bit for bit;
    against the option off (the three launches at 18 rows) the audio is within the README's bound, 3e-2."""
    from vibevoice_amd.synthetic import tokenizer_ids
    L = _lib.lib()
    TK = tokenizer_ids()
    D, E, S, X = TK.speech_diffusion_id, TK.speech_end_id, TK.speech_start_id, TK.eos_token_id
    B = 9
    cfg = _cfg()
    sd = _sd(cfg, 138)
    ids = torch.randint(0, 151000, (B, 12), generator=torch.Generator().manual_seed(5))
    mask = torch.ones(B, 12, dtype=torch.long)
    sched = [[D] * (3 + b % 3) + [E, S] + [D] * (2 + b % 2) + [X] for b in range(B)]
    outs = []
    for kw, graphs in ((dict(lm_attn_max_rows=32), (False, True)), ({}, (True,))):
        m = VibeVoiceForConditionalGenerationInference(cfg, sd, dev, max_batch=B, max_ctx=128, **kw)
        eng = m.engine
        assert L.vv_lm_attn_active(eng.h, 2 * B, eng.max_ctx) == (1 if kw else 0)
        assert m.lm_attn_max_rows == kw.get("lm_attn_max_rows") and L.vv_lm_attn_max_rows(eng.h) == (32 if kw else 16)
        m.set_ddpm_inference_steps(5)
        for use_graphs in graphs:
            torch.manual_seed(77)
            o = m.generate(input_ids=ids, attention_mask=mask, tokenizer=TK, cfg_scale=1.3, forced_tokens=sched,
                           use_graphs=use_graphs, show_progress_bar=False)
            outs.append((o.sequences.clone().cpu(), [a.clone().cpu() for a in o.speech_outputs]))
        assert len(m._graph_cache) >= 1
        eng.check_sync()
        assert_counters_consistent(eng)
        eng.close()
        del m, eng
        gc.collect()
    (seq_e, au_e), (seq_g, au_g), (seq_0, au_0) = outs
    assert torch.equal(seq_e, seq_g) and torch.equal(seq_e, seq_0)
    for b in range(B):
        assert torch.isfinite(au_e[b].float()).all() and au_e[b].float().abs().max() > 0
        assert torch.equal(bits(au_e[b]), bits(au_g[b])), b
        e = rel_err(au_g[b].float(), au_0[b].float())
        print(f"sample {b}: audio with the option vs without, rel {e:.3e}")
        assert e < 3e-2, (b, e)
