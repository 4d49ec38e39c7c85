"""Every stage of the streaming σ-VAE codec, and the streaming state itself, against a per-stage reference.

tests/test_gpu_codec.py compares the end of the whole chain (60+ bf16 layers) with the oracle at rel L2 < 3e-2.
Here each stage of both nets (acoustic decoder, semantic encoder) is compared on its own: after a vv_codec_step
the per-slot conv buffers hold every stage's input rows, output rows and histories (vv_diag_codec_layout /
vv_diag_codec_state), so tests/codec_ref.py's float64 stage is run on the GPU's OWN stage input and pre-step
histories (teacher forcing) and the error is that stage's alone.  Compared per stage and active slot: the output
rows (the next transition's rows; the audio / the semantic features for the last stages, and the last stage's
rows kept as the head's history), every block's mixer history, the transition / head histories.

Bound: codec_ref.M_GPU x e_cpu(stage) per quantity (the output, each mixer's history, the head's) in each of
codec_ref's measures: per (slot, frame) the whole, the worst row, the worst 8-channel chunk and the first 6 rows,
and pooled over all checked (slot, frame) draws of a test the worst chunk and the first 6 rows.  e_cpu is the
bfloat16 stage against the float64 stage on the CPU (codec_ref.noise_floor, computed here at run time from a
CPU-only stream, never from a GPU output).  tests/test_codec_ref_cpu.py shows that a wrong history row, tap, gamma
chunk or roll misses that bound by 2 x or more in a quantity and measure asserted here.  The decoder's last block
rows are not compared (its one-launch last stage keeps their last 6, the head history, which is); the encoder's
are (the head buffer holds them).

Exact (torch.equal): an inactive slot's state does not move; the input-row copies; k_roll (rows [0, ctx) after the
step = rows [T, T + ctx) before the roll, T = 1 < ctx = 6 included); a reset zeroes one slot's histories only.

Forms (convnet_run picks one per stage by C and T): persistent stage (C = 2,048, one sample), XF_MIX GEMVs,
k_mix + GEMMs, wide clusters (C = 256 / 512), k_block, tiles (C <= 128).  The cases below reach each one, and the
hand-over test runs one frame in the default forms and the next in the launch-per-block forms on the same state.

Measured on an MI355X, M_GPU = 2 (chosen after this run; the worst ratio of any measure, quantity, slot and frame is
1.55).  Per (net, stage): e_cpu (as the GPU host's CPU gave it) and the bound for the stage output's whole-stage
rel L2, then per case the worst
GPU whole-stage rel L2 of the output and the worst GPU error / e_cpu over all quantities and measures.  Cases:
one / many = the default forms (persistent stage or XF_MIX GEMVs, wide clusters, tiles) with one slot / the
three-slot schedule; block = stage, wide, tile off (XF_MIX, k_mix + GEMM, k_block); gemm = + mix fusion off
(k_mix + GEMMs everywhere); reset; hand = default forms, per-block forms, default forms on one state.
  net stage  e_cpu    bound   | one            | many           | block          | gemm           | reset          | hand
  dec 0      8.33e-03 1.67e-02 | 8.00e-03 1.39  | 8.05e-03 1.20  | 8.05e-03 1.20  | 8.05e-03 1.20  | 8.21e-03 1.37  | 7.88e-03 1.34
  dec 1      5.83e-03 1.17e-02 | 5.73e-03 1.05  | 5.63e-03 1.03  | 5.63e-03 1.03  | 5.63e-03 1.03  | 5.97e-03 1.51  | 5.87e-03 1.05
  dec 2      5.54e-03 1.11e-02 | 5.48e-03 1.03  | 5.43e-03 1.01  | 5.43e-03 1.01  | 5.43e-03 1.01  | 5.46e-03 1.19  | 5.52e-03 1.03
  dec 3      5.22e-03 1.04e-02 | 5.20e-03 1.04  | 5.19e-03 1.08  | 5.19e-03 1.08  | 5.19e-03 1.08  | 5.21e-03 1.13  | 5.16e-03 1.13
  dec 4      5.08e-03 1.02e-02 | 5.02e-03 1.22  | 5.04e-03 1.18  | 5.04e-03 1.18  | 5.04e-03 1.18  | 5.04e-03 1.16  | 5.04e-03 1.06
  dec 5      4.62e-03 9.24e-03 | 4.60e-03 1.07  | 4.63e-03 1.08  | 4.62e-03 1.08  | 4.62e-03 1.08  | 4.63e-03 1.15  | 4.60e-03 1.10
  dec 6      4.94e-03 9.88e-03 | 4.95e-03 1.49  | 4.86e-03 1.53  | 4.93e-03 1.53  | 4.93e-03 1.53  | 4.92e-03 1.33  | 4.97e-03 1.08
  enc 0      4.42e-03 8.84e-03 | 4.39e-03 1.00  | 4.40e-03 1.24  | 4.40e-03 1.24  | 4.40e-03 1.24  | 4.39e-03 1.20  | 4.38e-03 1.55
  enc 1      4.50e-03 9.01e-03 | 4.52e-03 1.11  | 4.52e-03 1.10  | 4.53e-03 1.08  | 4.53e-03 1.08  | 4.52e-03 1.04  | 4.52e-03 1.12
  enc 2      4.52e-03 9.04e-03 | 4.49e-03 1.10  | 4.52e-03 1.09  | 4.52e-03 1.09  | 4.52e-03 1.09  | 4.52e-03 1.18  | 4.50e-03 1.07
  enc 3      4.51e-03 9.01e-03 | 4.48e-03 1.16  | 4.48e-03 1.03  | 4.48e-03 1.07  | 4.48e-03 1.07  | 4.52e-03 1.10  | 4.48e-03 1.08
  enc 4      4.50e-03 9.00e-03 | 4.48e-03 1.02  | 4.47e-03 1.04  | 4.47e-03 1.03  | 4.47e-03 1.03  | 4.51e-03 1.13  | 4.46e-03 1.07
  enc 5      4.47e-03 8.95e-03 | 4.48e-03 1.03  | 4.44e-03 1.03  | 4.46e-03 1.03  | 4.46e-03 1.03  | 4.51e-03 1.03  | 4.43e-03 1.16
  enc 6      7.85e-03 1.57e-02 | 6.14e-03 1.27  | 6.89e-03 1.43  | 7.21e-03 1.44  | 7.21e-03 1.44  | 7.66e-03 1.37  | 6.77e-03 1.45
The worst ratios are in the measures that are maxima or cover few values: dec 6 the first 6 audio samples of one
frame (9.2e-3 vs 6.0e-3), enc 0 the worst of 3,200 rows (1.85e-2 vs 1.19e-2), dec 1 the worst chunk (2.07e-2
vs 1.37e-2).
"""
import ctypes
import gc

import pytest
import torch

import codec_ref as cr
from oracle import codec as ocodec
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
dev = "cuda"
NSLOT = 3
PARTS = ("decoder", "encoder")

@pytest.fixture(autouse=True)
def _collect_engines():
    """The persistent codec stage runs only while its context is the device's
    only one registered for persistent kernels: drop engines of earlier tests."""
    gc.collect()
    yield


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


@pytest.fixture(scope="module")
def G():
    """The real codec on a tiny LM, its CPU weights, and the CPU noise floor e_cpu per (part, stage) (two samples,
    three frames, decoder -> encoder, all on the CPU) with the float64 weights it cast."""
    cfg = tiny_config(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    g = dict(cfg=cfg, sd_all=sd)
    g["sd"] = {"decoder": sub(sd, "model.acoustic_tokenizer."), "encoder": sub(sd, "model.semantic_tokenizer.")}
    g["dims"] = {"decoder": ocodec.codec_dims(cfg.acoustic_tokenizer_config, "decoder"),
                 "encoder": ocodec.codec_dims(cfg.semantic_tokenizer_config, "encoder")}
    g["scale"], g["bias"] = sd["model.speech_scaling_factor"], sd["model.speech_bias_factor"]
    gen = torch.Generator().manual_seed(41)
    lats = [torch.randn(2, 64, generator=gen).bfloat16() for _ in range(3)]
    g["w64"] = {}
    g["floor"] = cr.noise_floor(g["sd"], g["dims"], lats, g["scale"], g["bias"], 2, g["w64"])
    return g


def make_engine(G):
    gc.collect()
    eng = Engine(G["cfg"], G["sd_all"], dev, max_batch=NSLOT, max_ctx=64)
    L = _lib.lib()
    lay = []
    for net in (0, 1):
        w = (ctypes.c_int * 512)()
        assert L.vv_diag_codec_layout(eng.h, net, w, 3) != 0            # capacity short: fails
        _lib.check(L.vv_diag_codec_layout(eng.h, net, w, 512), "diag_codec_layout")
        lay.append(cr.parse_layout(list(w)))
    return eng, lay


def dump(eng, lay):
    """[net][slot] -> split_dump()'s buffers on the CPU."""
    L = _lib.lib()
    out = []
    for net in (0, 1):
        ne = cr.layout_elems(lay[net])
        per = []
        for s in range(NSLOT):
            t = torch.empty(ne, dtype=torch.bfloat16, device=dev)
            _lib.check(L.vv_diag_codec_state(eng.h, net, s, ctypes.c_void_p(t.data_ptr()), ne), "diag_codec_state")
            per.append(cr.split_dump(t.cpu(), lay[net]))
        out.append(per)
    return out


def step(eng, G, slots, lat):
    n = len(slots)
    sl = torch.tensor(slots, dtype=torch.int32, device=dev)
    audio = torch.empty(n, G["cfg"].hop, dtype=torch.bfloat16, device=dev)
    sem = torch.empty(n, 128, dtype=torch.bfloat16, device=dev)
    eng.codec_step(sl, lat.to(dev), audio, sem)
    torch.cuda.synchronize()
    return audio.cpu(), sem.cpu()


def check_exact(G, lay, pre, post, slots, lat, audio):
    """The state invariants that hold bit for bit."""
    for net in (0, 1):
        for s in range(NSLOT):
            if s not in slots:
                for a, b in zip(pre[net][s], post[net][s]):
                    assert torch.equal(a, b), ("inactive slot moved", net, s)
    assert lat.dtype == torch.bfloat16
    z = lat / G["scale"] - G["bias"]                     # bf16(bf16(lat / scaling) - bias)
    for r, s in enumerate(slots):
        b = lay[0][0]
        assert b["kind"] == "stem" and torch.equal(post[0][s][0][b["ctx"]: b["ctx"] + 1], z[r: r + 1]), ("latent rows", s)
        b = lay[1][0]
        assert torch.equal(post[1][s][0][b["ctx"]: b["ctx"] + b["T"], 0], audio[r]), ("encoder input rows", s)
        for net in (0, 1):
            for n, b in enumerate(lay[net]):
                want = cr.rolled(pre[net][s][n], post[net][s][n], b)
                assert torch.equal(post[net][s][n][: b["ctx"]], want), ("roll", net, s, b)


def note(seen, bad, tag, part, i, q, m, v, floor):
    ratio = v / floor[q][m]
    k = (part, i)
    cur = seen.setdefault(k, {"whole": 0.0, "worst": (0.0, "")})
    if q == "out" and m == 0:
        cur["whole"] = max(cur["whole"], v)
    cur["worst"] = max(cur["worst"], (ratio, f"{q}/{cr.MEASURES[m]}"))
    if not ratio <= cr.M_GPU:
        bad.append((tag, part, i, q, cr.MEASURES[m], v, floor[q][m], ratio))


def check_stages(G, lay, pre, post, slots, check, audio, sem, tag, seen, pools, want_taps):
    """Every stage of both nets for the slots in `check`: the float64 stage on the GPU's own input rows and pre-step
    histories vs what the GPU left, in the per-draw measures; pools: {(part, stage): codec_ref.Pool} receives every
    draw for the pooled ones.  seen: the worst figures per (part, stage)."""
    rows = [r for r, s in enumerate(slots) if s in check]
    cs = [slots[r] for r in rows]
    n = len(cs)
    bad = []
    for net, part in enumerate(PARTS):
        dims, L = G["dims"][part], lay[net]
        nst = len(dims["depths"])
        pre_b, post_b = [pre[net][s] for s in cs], [post[net][s] for s in cs]
        for i in range(nst):
            keys = cr.stage_keys(part, dims, i)
            hist = cr.hist_from_dumps(pre_b, L, part, dims, keys)
            nin = cr.find_buf(L, part, cr.pre_key(part, i))
            x_in = cr.new_rows(post_b, L, nin)
            ref = cr.run_stage(G["w64"][(part, i)], dims, part, i, x_in, hist, torch.float64)
            got = {"hist": cr.hist_from_dumps(post_b, L, part, dims, keys), "final": None}
            if i < nst - 1:
                got["x"] = cr.new_rows(post_b, L, cr.find_buf(L, part, cr.pre_key(part, i + 1)), ref["x"].shape[-1])
            elif part == "decoder":
                # the one-launch last stage keeps only the last 6 of its rows: the head history, compared below
                got["final"], got["x"] = audio[rows][:, None, :], None
            else:
                # the encoder's head conv is a launch of its own: the head buffer holds the last stage's rows
                got["final"] = sem[rows][:, :, None]
                got["x"] = cr.new_rows(post_b, L, cr.find_buf(L, part, cr.head_key(part)), ref["x"].shape[-1])
            # the transition's own history is a copy of input rows: exact
            pk = cr.pre_key(part, i)
            keep = L[nin]["ctx"]
            assert torch.equal(got["hist"][pk][:, :, -keep:].double(), ref["hist"][pk][:, :, -keep:]), (tag, pk)
            floor = G["floor"][(part, i)]
            for q, v in cr.stage_errs(got, ref, n).items():
                for m in range(cr.PER_DRAW):
                    note(seen, bad, tag, part, i, q, m, v[m], floor)
            for idx in range(n):
                pools.setdefault((part, i), cr.Pool()).add(got, ref, idx)
            # the history taps are live (slots with a frame behind them): every block's history is non-zero
            # and adds a non-zero term to the reference's depthwise conv
            taps = cr.hist_taps(G["w64"][(part, i)], dims, part, i, hist)
            for idx, s in enumerate(cs):
                for j in range(dims["depths"][i] if s in want_taps else 0):
                    assert hist[cr.mixer_key(part, i, j)][idx].abs().sum() > 0, (tag, part, i, j, s)
                    assert taps[j][idx].norm() > 0, (tag, part, i, j, s)
    return bad


def check_pools(G, pools, tag, seen):
    """The pooled measures over every draw of the stream (at least 3, as many as e_cpu's pools hold)."""
    bad = []
    for (part, i), pool in pools.items():
        for q, v in pool.result().items():
            for m in range(2):
                note(seen, bad, tag, part, i, q, cr.PER_DRAW + m, v[m], G["floor"][(part, i)])
    return bad


def report(seen, G, tag):
    for (part, i), v in sorted(seen.items()):
        e = G["floor"][(part, i)]["out"][0]
        print(f"{tag} {part} stage {i}: out whole gpu {v['whole']:.2e} e_cpu {e:.2e} bound {cr.M_GPU * e:.2e}; "
              f"worst of all {v['worst'][0]:.2f} x e_cpu ({v['worst'][1]})")
    print(f"{tag}: worst ratio {max(v['worst'][0] for v in seen.values()):.2f} (bound {cr.M_GPU})")


def stream(G, eng, lay, sched, tag, seed, full_frame=1, before_frame=None):
    """Run the schedule; exact checks on every frame and slot; stages for all slots in frame `full_frame` and
    for the first active slot in the others (the float64 reference is 1.6 GMAC per net, sample and frame)."""
    gen = torch.Generator().manual_seed(seed)
    eng.codec_reset(torch.arange(NSLOT, dtype=torch.int32, device=dev))
    pre = dump(eng, lay)
    seen, pools, bad = {}, {}, []
    touched = set()
    draws = 0
    for f, slots in enumerate(sched):
        if before_frame:
            pre = before_frame(f, pre, touched) or pre
        lat = torch.randn(len(slots), 64, generator=gen).bfloat16()
        audio, sem = step(eng, G, slots, lat)
        post = dump(eng, lay)
        check_exact(G, lay, pre, post, slots, lat, audio)
        check = set(slots) if f == full_frame else {slots[0]}
        draws += len(check)
        bad += check_stages(G, lay, pre, post, slots, check, audio, sem, f"{tag} frame {f}", seen, pools,
                            check & touched)
        touched |= set(slots)
        pre = post
    eng.check_sync()
    assert draws >= 3
    bad += check_pools(G, pools, tag, seen)
    report(seen, G, tag)
    assert not bad, bad
    return seen


TILE, WIDE, STAGE, BLOCKS, GEMMS = range(5)     # vv_diag_codec_plan's routes
CHANS = ([2048, 1024, 512, 256, 128, 64, 32], [32, 64, 128, 256, 512, 1024, 2048])   # decoder, encoder
# the stages the mixer fits fc1's prologue at (<= 16 rows of <= 4 samples within 96 KB of LDS): (C, T) -> the n
XF_MIX = {(2048, 1): (1, 2), (1024, 8): (1,)}


def check_plan(eng, n, forms, fusion):
    """vv_diag_codec_plan of both nets at n samples against the routes the case's docstring names: forms = the
    one-launch stages (persistent, clusters, tiles) are on; fusion = vv_codec_mix_fusion's mask."""
    L = _lib.lib()
    wide_dec = 0
    for net in (0, 1):
        w = (ctypes.c_int * 64)()
        assert L.vv_diag_codec_plan(eng.h, net, n, w, 43) != 0                   # capacity short: fails
        _lib.check(L.vv_diag_codec_plan(eng.h, net, n, w, 64), "diag_codec_plan")
        assert w[0] == 7
        st = [tuple(w[2 + 6 * i: 8 + 6 * i]) for i in range(7)]
        print(f"codec plan net {net} n={n} forms={forms} fusion={fusion}: own_head {w[1]} {st}")
        for i, (route, pre, post, own_pre, xf_mix, R) in enumerate(st):
            C = CHANS[net][i]
            T = 3200 * 32 // C if C <= 128 else {256: 200, 512: 40, 1024: 8, 2048: 1}[C]
            if C <= 128:                         # tiles; k_block per Block1D with bit 1 of the mask, else GEMMs
                want = (TILE,) if forms else (BLOCKS,) if fusion & 2 else (GEMMS,)
            elif C <= 512:
                # clusters: 3 x 16 x n workgroups at C = 512, 13 x 8 x n at C = 256; the MI355X holds one 512-thread
                # cluster workgroup on each of its 256 CUs, so C = 256 at n = 3 (312 workgroups) is not resident
                # and keeps its GEMMs
                want = (WIDE,) if forms and (C == 512 or n <= 2) else (GEMMS,)
            else:                                # the persistent stage takes one sample
                want = (STAGE,) if forms and n == 1 else (GEMMS,)
            assert route in want, (net, i, n, st[i], want)
            assert xf_mix == int(route == GEMMS and bool(fusion & 1) and n in XF_MIX.get((C, T), ())), (net, i, n, st[i])
            assert R == (0 if route < BLOCKS else max(1, min(T, 2048 // C))), (net, i, n, st[i])
            # the decoder's 2x transposed convs / head conv, the encoder's stem / 2x strided convs ride in the tiles
            fused = route == TILE and C <= (64 if net == 0 else 128)
            assert own_pre == int(not fused) and (pre != 0) == fused and post == int(route == TILE and net == 0 and i == 6)
        assert w[1] == int(not (net == 0 and st[6][0] == TILE))
        if net == 0:
            if n == 1:
                assert L.vv_codec_stage_active(eng.h) == int(st[0][0] == STAGE)
            assert L.vv_codec_wide_active(eng.h, n) == int(any(s[0] == WIDE for s in st))


SCHED = [[0, 2], [0, 1, 2], [2]]
CASES = [("default-one", [[1]] * 3, None, (1, 1)),
         ("default-many", SCHED, None, (1, 1)),
         ("per-block", SCHED, 3, (0, 0)),
         ("gemm", SCHED, 0, (0, 0))]


@pytest.mark.parametrize("name,sched,fusion,active", CASES, ids=[c[0] for c in CASES])
def test_stages_and_state(G, name, sched, fusion, active):
    """default-one: persistent stage, wide, tile.  default-many: XF_MIX GEMVs, wide at n = 2 / 3 (C = 256: n = 2 only,
    k_mix + GEMMs at n = 3), tile.
    per-block (stage, wide, tile off): k_block, XF_MIX, k_mix + GEMM.  gemm (+ mix fusion off): k_mix + GEMMs."""
    L = _lib.lib()
    eng, lay = make_engine(G)
    try:
        if fusion is not None:
            L.vv_codec_stage(0)
            L.vv_codec_wide(0)
            L.vv_codec_tile(0)
            L.vv_codec_mix_fusion(fusion)
        assert L.vv_codec_stage_active(eng.h) == active[0]
        for n in sorted({len(s) for s in sched}):
            assert L.vv_codec_wide_active(eng.h, n) == active[1], n
            check_plan(eng, n, fusion is None, 3 if fusion is None else fusion)
        stream(G, eng, lay, sched, name, 51)
    finally:
        L.vv_codec_stage(1)
        L.vv_codec_wide(1)
        L.vv_codec_tile(1)
        L.vv_codec_mix_fusion(3)
        eng.close()


def test_reset_one_slot(G):
    """speech_end of slot 1 mid-stream: its history rows are zero in every buffer of both nets, the other slots'
    state is bit-identical, and its next frame matches the reference started from zero state."""
    eng, lay = make_engine(G)
    try:
        def before(f, pre, touched):
            if f != 2:
                return None
            eng.codec_reset(torch.tensor([1], dtype=torch.int32, device=dev))
            now = dump(eng, lay)
            for net in (0, 1):
                for s in range(NSLOT):
                    for n, b in enumerate(lay[net]):
                        if s == 1:
                            assert not now[net][s][n][: b["ctx"]].any(), ("reset left history", net, n)
                        else:
                            assert torch.equal(now[net][s][n], pre[net][s][n]), ("reset moved another slot", net, s, n)
            assert any(pre[0][1][n][: b["ctx"]].any() for n, b in enumerate(lay[0]))      # there was state to zero
            touched.discard(1)
            return now
        # frame 2 checks slot 1 (first active): its pre-step histories are the zeros asserted above
        stream(G, eng, lay, [[0, 1, 2], [1, 0], [1, 2]], "reset", 53, full_frame=0, before_frame=before)
    finally:
        eng.close()


def test_form_hand_over(G):
    """One frame in the default forms (persistent stage / wide clusters / tiles), the next with all three off
    (XF_MIX GEMVs, k_mix + GEMMs, k_block) on the same state, and back: the state one form writes is the state
    every other form reads (only the last 6 normalised rows of a mixer buffer are portable)."""
    L = _lib.lib()
    eng, lay = make_engine(G)
    try:
        def before(f, pre, touched):
            on = 0 if f == 1 else 1
            L.vv_codec_stage(on)
            L.vv_codec_wide(on)
            L.vv_codec_tile(on)
            assert L.vv_codec_stage_active(eng.h) == on and L.vv_codec_wide_active(eng.h, 1) == on
            check_plan(eng, 1, bool(on), 3)
        stream(G, eng, lay, [[1], [1], [1]], "hand-over", 57, before_frame=before)
    finally:
        L.vv_codec_stage(1)
        L.vv_codec_wide(1)
        L.vv_codec_tile(1)
        eng.close()


def test_first_block_norm_rows_same_bits_in_every_form(G):
    """The mixer norm is one rounding chain for every kernel form (csrc/codec_dev.h: cb_ss8, the form's row sum,
    cb_norm).  Block 0's mixer history rows of a stage are norm(x) of the stage input and depend on nothing else
    (no fc1, GELU or fc2), so with the stage input held fixed they must agree bit for bit between the forms.  From a
    reset state one frame of slot 0 is run per arm, each arm with one switch away from the default; the stages
    upstream of the one compared run the same kernels in both runs, and the compared stage's input rows (the rows
    its transition buffer holds) are asserted equal first, so a failure says which side moved.
      dec stage 0 (C = 2,048, T = 1): persistent stage | XF_MIX GEMV (vv_codec_stage 0) | k_mix (+ mix fusion 0)
      dec stage 2 (C = 512, T = 40):  wide clusters | k_mix + GEMM (vv_codec_wide 0)
      dec stage 4 (C = 128, T = 400): tile | k_block (vv_codec_tile 0)
    Rows compared: only the last min(T, 6) of this frame's rows [ctx, ctx + T) -- 1 of 1, 6 of 40 and 6 of 400 --
    the rows the next frame reads; the one-launch forms store no others (include/vibevoice_hip_diag.h,
    vv_diag_codec_state), so the earlier rows of a frame are pinned only through the stage tests above.
    On the commit before codec_dev.h every pair was already exact (0 differing values of 2,048 / 3,072 / 768 in
    the three stages, k_mix arm included): all four pairs assert torch.equal."""
    L = _lib.lib()
    eng, lay = make_engine(G)
    lat = torch.randn(1, 64, generator=torch.Generator().manual_seed(61)).bfloat16()
    ne = cr.layout_elems(lay[0])

    def run(stage=1, wide=1, tile=1, fusion=3):
        L.vv_codec_stage(stage)
        L.vv_codec_wide(wide)
        L.vv_codec_tile(tile)
        L.vv_codec_mix_fusion(fusion)
        eng.codec_reset(torch.arange(NSLOT, dtype=torch.int32, device=dev))
        step(eng, G, [0], lat)
        t = torch.empty(ne, dtype=torch.bfloat16, device=dev)
        _lib.check(L.vv_diag_codec_state(eng.h, 0, 0, ctypes.c_void_p(t.data_ptr()), ne), "diag_codec_state")
        w = (ctypes.c_int * 64)()
        _lib.check(L.vv_diag_codec_plan(eng.h, 0, 1, w, 64), "diag_codec_plan")
        return cr.split_dump(t.cpu(), lay[0]), [w[2 + 6 * i] for i in range(7)], [w[6 + 6 * i] for i in range(7)]

    def rows(bufs, i):
        b_in = lay[0][cr.find_buf(lay[0], "decoder", cr.pre_key("decoder", i))]
        b_mx = lay[0][cr.find_buf(lay[0], "decoder", cr.mixer_key("decoder", i, 0))]
        x = bufs[lay[0].index(b_in)][b_in["ctx"]: b_in["ctx"] + b_in["T"]]
        T, c = b_mx["T"], b_mx["ctx"]
        return x, bufs[lay[0].index(b_mx)][c + max(T - 6, 0): c + T]

    try:
        base, route, _ = run()
        assert (route[0], route[2], route[4]) == (STAGE, WIDE, TILE), route
        arms = [("stage|xf_mix", 0, dict(stage=0), GEMMS, 1), ("stage|k_mix", 0, dict(stage=0, fusion=0), GEMMS, 0),
                ("wide|k_mix", 2, dict(wide=0), GEMMS, 0), ("tile|k_block", 4, dict(tile=0), BLOCKS, 0)]
        for name, i, kw, want_route, want_xf in arms:
            other, route, xf = run(**kw)
            assert (route[i], xf[i]) == (want_route, want_xf), (name, route, xf)
            (xa, na), (xb, nb) = rows(base, i), rows(other, i)
            assert na.abs().sum() > 0 and na.shape == nb.shape and na.shape[0] == min(6, lay[0][cr.find_buf(
                lay[0], "decoder", cr.mixer_key("decoder", i, 0))]["T"])
            print(f"{name}: stage {i} input values that differ {int((xa != xb).sum())} of {xa.numel()}, "
                  f"norm rows {int((na != nb).sum())} of {na.numel()}")
            assert torch.equal(xa, xb), (name, "the stage input moved")
            assert torch.equal(na, nb), (name, "block 0's mixer norm rows differ")
        eng.check_sync()
    finally:
        L.vv_codec_stage(1)
        L.vv_codec_wide(1)
        L.vv_codec_tile(1)
        L.vv_codec_mix_fusion(3)
        eng.close()


def test_diag_state_rejects_short_capacity(G):
    eng, lay = make_engine(G)
    try:
        L = _lib.lib()
        ne = cr.layout_elems(lay[0])
        t = torch.full((ne,), 7.0, dtype=torch.bfloat16, device=dev)
        assert L.vv_diag_codec_state(eng.h, 0, 0, ctypes.c_void_p(t.data_ptr()), ne - 1) != 0
        assert L.vv_diag_codec_state(eng.h, 0, NSLOT, ctypes.c_void_p(t.data_ptr()), ne) != 0
        assert bool((t == 7.0).all())                                    # nothing written
        kinds = [b["kind"] for b in lay[0]]
        assert kinds[0] == "stem" and kinds[-1] == "head" and kinds.count("tr") == 6 and kinds.count("mix") == 26
        assert [(b["ctx"], b["T"], b["C"]) for b in lay[1] if b["kind"] == "tr"][0] == (2, 3200, 32)
    finally:
        eng.close()
