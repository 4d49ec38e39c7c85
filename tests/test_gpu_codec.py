"""Streaming σ-VAE codec step on the GPU (vv_codec_step / vv_codec_reset) vs
the CPU oracle at the real 1.5B codec shapes (acoustic decoder 64 -> 3200
samples per frame, semantic encoder 3200 -> 128, both connectors).

Covers: per-slot streaming state over several frames, a sample that skips a
frame (its state must not move), set_to_zero on speech_end, and the
acoustic+semantic connector sum written into the next-embedding rows.
Tolerance (bf16 model, 60+ layers deep, different GEMM accumulation order
than the reference / oracle): rel L2 < 3e-2 and cosine > 0.999.

A failure here says the chain is off; tests/test_gpu_codec_stages.py says which
stage, block and slot (each stage against its own float64 reference, and the
streaming state bit for bit).
"""
import pytest
import torch

from gpu_util import cos, rel_err
from oracle import codec as ocodec
from oracle import lm as olm
from sync_counters import assert_counters_consistent
from tiny import tiny_config
from vibevoice_amd.engine import Engine
from vibevoice_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(autouse=True)
def _collect_engines():
    """The persistent codec stage runs only while its context is the device's
    only one registered for persistent kernels: drop engines of earlier tests."""
    import gc
    gc.collect()
    yield


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def connector(sd, p, x):
    F = torch.nn.functional
    y = F.linear(x, sd[p + "fc1.weight"], sd[p + "fc1.bias"])
    y = olm.rms(y, sd[p + "norm.weight"], 1e-6)
    return F.linear(y, sd[p + "fc2.weight"], sd[p + "fc2.bias"])


def test_codec_stream_real_shapes():
    cfg = tiny_config(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    eng = Engine(cfg, sd, dev, max_batch=3, max_ctx=64)
    hop = cfg.hop
    H = cfg.decoder_config.hidden_size
    dd = ocodec.codec_dims(cfg.acoustic_tokenizer_config, "decoder")
    ed = ocodec.codec_dims(cfg.semantic_tokenizer_config, "encoder")
    sd_a, sd_s = sub(sd, "model.acoustic_tokenizer."), sub(sd, "model.semantic_tokenizer.")
    st_a, st_s = ocodec.StreamState(3), ocodec.StreamState(3)
    s_f, b_f = sd["model.speech_scaling_factor"], sd["model.speech_bias_factor"]
    g = torch.Generator().manual_seed(5)
    sched = [[0, 2], [0, 2], [2], [0, 1, 2]]
    worst = []
    for step, slots in enumerate(sched):
        n = len(slots)
        lat = torch.randn(n, 64, generator=g).bfloat16()
        # --- GPU
        d_slots = torch.tensor(slots, dtype=torch.int32, device=dev)
        audio = torch.empty(n, hop, dtype=torch.bfloat16, device=dev)
        sem = torch.empty(n, 128, dtype=torch.bfloat16, device=dev)
        emb = torch.zeros(3, H, dtype=torch.bfloat16, device=dev)
        eng.codec_step(d_slots, lat.to(dev), audio, sem, emb, d_slots)
        # --- oracle (modeling_vibevoice_inference.py:651-687)
        idx = torch.tensor(slots)
        z = (lat / s_f - b_f).unsqueeze(-1)
        a_ref = ocodec.decode(sd_a, dd, z, st_a, idx)
        s_ref = ocodec.encode(sd_s, ed, a_ref, st_s, idx)[:, 0]
        e_ref = connector(sd, "model.acoustic_connector.", lat) + connector(sd, "model.semantic_connector.", s_ref)
        torch.cuda.synchronize()
        for name, got, ref in (("audio", audio, a_ref[:, 0]), ("sem", sem, s_ref), ("emb", emb[idx.to(dev)], e_ref)):
            e, c = rel_err(got, ref), cos(got, ref)
            worst.append((step, name, e, c))
            print(f"step {step} {name}: rel_err {e:.3e} cos {c:.6f}")
            assert e < 3e-2 and c > 0.999, (step, name, e, c)
        if step == 1:   # speech_end for slot 0 (set_to_zero, :556-560)
            eng.codec_reset(torch.tensor([0], dtype=torch.int32, device=dev))
            st_a.zero(torch.tensor([0]))
            st_s.zero(torch.tensor([0]))


@pytest.mark.parametrize("n,mask", [(1, 1), (1, 2), (1, 3), (2, 3), (3, 3)])
def test_mix_fusion_bit_exact(n, mask):
    """The codec Block1D mixer folded into fc1's prologue (XF_MIX, rows <= 16)
    must give the separate k_mix + fc1 path's bits, state included: three
    streamed frames per mode, then audio / semantic features / embeddings and
    the next frame compared exactly.  n = 3 exceeds the fused form's LDS and
    runs XF_MIX unfused in both modes.  mask: which fusions are on (bit 0
    XF_MIX, bit 1 k_block)."""
    from vibevoice_amd import _lib
    cfg = tiny_config(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    eng = Engine(cfg, sd, dev, max_batch=3, max_ctx=64)
    H = cfg.decoder_config.hidden_size
    g = torch.Generator().manual_seed(7)
    lats = [torch.randn(n, 64, generator=g).bfloat16().to(dev) for _ in range(4)]
    slots = torch.arange(n, dtype=torch.int32, device=dev)
    outs = {}
    _lib.lib().vv_codec_stage(0)   # the stage kernel would replace the n = 1 T = 1 stages in both modes
    try:
        for fuse in (0, mask):
            _lib.lib().vv_codec_mix_fusion(fuse)
            eng.codec_reset(slots)
            res = []
            for lat in lats:
                audio = torch.empty(n, cfg.hop, dtype=torch.bfloat16, device=dev)
                sem = torch.empty(n, 128, dtype=torch.bfloat16, device=dev)
                emb = torch.zeros(n, H, dtype=torch.bfloat16, device=dev)
                eng.codec_step(slots, lat, audio, sem, emb, slots)
                res += [audio, sem, emb]
            torch.cuda.synchronize()
            outs[fuse] = res
    finally:
        _lib.lib().vv_codec_mix_fusion(3)
        _lib.lib().vv_codec_stage(1)
    for i, (a, b) in enumerate(zip(outs[0], outs[mask])):
        assert torch.equal(a, b), (n, i, (a.float() - b.float()).abs().max().item())


@pytest.mark.parametrize("n", [3, 4, 5, 6, 8])
def test_codec_stream_batch_sizes(n):
    """The streaming codec at the real shapes with n = 3..8 diffusing rows
    (configs[2]: B = 8), slots scattered over a max_batch 8 engine: three
    frames vs the oracle, per row."""
    cfg = tiny_config(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    eng = Engine(cfg, sd, dev, max_batch=8, max_ctx=64)
    hop = cfg.hop
    dd = ocodec.codec_dims(cfg.acoustic_tokenizer_config, "decoder")
    ed = ocodec.codec_dims(cfg.semantic_tokenizer_config, "encoder")
    sd_a, sd_s = sub(sd, "model.acoustic_tokenizer."), sub(sd, "model.semantic_tokenizer.")
    st_a, st_s = ocodec.StreamState(8), ocodec.StreamState(8)
    s_f, b_f = sd["model.speech_scaling_factor"], sd["model.speech_bias_factor"]
    g = torch.Generator().manual_seed(11)
    slots = sorted(torch.randperm(8, generator=g)[:n].tolist())
    eng.codec_reset(torch.arange(8, dtype=torch.int32, device=dev))
    bad = []
    for step in range(3):
        lat = torch.randn(n, 64, generator=g).bfloat16()
        d_slots = torch.tensor(slots, dtype=torch.int32, device=dev)
        audio = torch.empty(n, hop, dtype=torch.bfloat16, device=dev)
        sem = torch.empty(n, 128, dtype=torch.bfloat16, device=dev)
        eng.codec_step(d_slots, lat.to(dev), audio, sem)
        idx = torch.tensor(slots)
        a_ref = ocodec.decode(sd_a, dd, (lat / s_f - b_f).unsqueeze(-1), st_a, idx)[:, 0]
        s_ref = ocodec.encode(sd_s, ed, a_ref[:, None], st_s, idx)[:, 0]
        torch.cuda.synchronize()
        for r in range(n):
            ea, es = rel_err(audio[r], a_ref[r]), rel_err(sem[r], s_ref[r])
            print(f"n {n} step {step} row {r} (slot {slots[r]}): audio rel {ea:.3e} sem rel {es:.3e}")
            if not (ea < 3e-2 and es < 3e-2):
                bad.append((step, r, ea, es))
    assert not bad, bad


def test_codec_stage_persistent_launch():
    """The C = 2,048 T = 1 stages (acoustic decoder's first, semantic encoder's
    last; 8 Block1Ds each) as ONE persistent launch (codec_stage.hip) vs the
    launch-per-GEMV path (XF_MIX fc1 + fc2 GEMVs) and vs the oracle, one
    sample over four streamed frames (the stage's conv buffers carry state from
    frame to frame): the front half is XF_MIX's arithmetic, fc1 / fc2 sum in
    another order, so within bf16 of both (the codec tolerance, rel L2 < 3e-2,
    vs each: the audio runs through 60+ bf16 layers after the stage, and the two
    paths differ by as much as each differs from the oracle, 1.4e-2 vs 1.6e-2
    at frame 0), and bitwise equal run to run."""
    from vibevoice_amd import _lib
    L = _lib.lib()
    cfg = tiny_config(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    eng = Engine(cfg, sd, dev, max_batch=2, max_ctx=64)
    assert L.vv_codec_stage_active(eng.h) == 1
    H = cfg.decoder_config.hidden_size
    dd = ocodec.codec_dims(cfg.acoustic_tokenizer_config, "decoder")
    ed = ocodec.codec_dims(cfg.semantic_tokenizer_config, "encoder")
    sd_a, sd_s = sub(sd, "model.acoustic_tokenizer."), sub(sd, "model.semantic_tokenizer.")
    s_f, b_f = sd["model.speech_scaling_factor"], sd["model.speech_bias_factor"]
    g = torch.Generator().manual_seed(13)
    lats = [torch.randn(1, 64, generator=g).bfloat16() for _ in range(4)]
    slot = torch.tensor([1], dtype=torch.int32, device=dev)
    outs = {}
    try:
        for mode in (1, 0, 1, 3):   # 3: the stage with round 5's whole-block weight stream
            L.vv_codec_stage(mode)
            assert L.vv_codec_stage_active(eng.h) == (mode & 1)
            eng.codec_reset(slot)
            res = []
            for lat in lats:
                audio = torch.empty(1, cfg.hop, dtype=torch.bfloat16, device=dev)
                sem = torch.empty(1, 128, dtype=torch.bfloat16, device=dev)
                emb = torch.zeros(2, H, dtype=torch.bfloat16, device=dev)
                eng.codec_step(slot, lat.to(dev), audio, sem, emb, slot)
                res.append((audio, sem, emb[1:2]))
            torch.cuda.synchronize()
            outs.setdefault(mode, []).append(res)
    finally:
        L.vv_codec_stage(1)
    eng.check_sync()
    assert_counters_consistent(eng)   # a clean run leaves every wait counter at a whole number of waits
    st_a, st_s = ocodec.StreamState(2), ocodec.StreamState(2)
    idx = torch.tensor([1])
    for f, lat in enumerate(lats):
        a_ref = ocodec.decode(sd_a, dd, (lat / s_f - b_f).unsqueeze(-1), st_a, idx)
        s_ref = ocodec.encode(sd_s, ed, a_ref, st_s, idx)[:, 0]
        e_ref = connector(sd, "model.acoustic_connector.", lat) + connector(sd, "model.semantic_connector.", s_ref)
        for k, (name, ref) in enumerate((("audio", a_ref[:, 0]), ("sem", s_ref), ("emb", e_ref))):
            got, base, again = outs[1][0][f][k], outs[0][0][f][k], outs[1][1][f][k]
            e_o, e_b = rel_err(got, ref), rel_err(got, base)
            print(f"frame {f} {name}: rel {e_o:.3e} vs oracle ({rel_err(base, ref):.3e} GEMV path), "
                  f"{e_b:.3e} vs the GEMV path")
            assert torch.equal(got, again), (f, name)
            assert torch.equal(got, outs[3][0][f][k]), (f, name)   # issue order only: same sums
            assert e_o < 3e-2 and cos(got, ref) > 0.999, (f, name, e_o)
            assert e_b < 3e-2 and cos(got, base) > 0.999, (f, name, e_b)


def test_codec_stage_only_for_the_devices_sole_context():
    """The persistent codec stage holds one workgroup per CU and waits grid-wide:
    with a second registered context on the device, both run the launch-per-GEMV
    path (the same streaming state carries on, within bf16 of the stage's), and
    the first returns to the stage when the second is destroyed (vv_ws_epoch
    bumps each time, so captured graphs are re-captured)."""
    from vibevoice_amd import _lib
    L = _lib.lib()
    cfg = tiny_config(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    a = Engine(cfg, sd, dev, max_batch=1, max_ctx=64)
    assert L.vv_codec_stage_active(a.h) == 1
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(17)
    lats = [torch.randn(1, 64, generator=g).bfloat16().to(dev) for _ in range(3)]

    def frames(eng):
        eng.codec_reset(slot)
        out = []
        for lat in lats:
            audio = torch.empty(1, cfg.hop, dtype=torch.bfloat16, device=dev)
            eng.codec_step(slot, lat, audio)
            out.append(audio)
        torch.cuda.synchronize()
        return out

    solo = frames(a)
    e0 = L.vv_ws_epoch()
    b = Engine(cfg, sd, dev, max_batch=1, max_ctx=64)
    assert L.vv_codec_stage_active(a.h) == 0 and L.vv_codec_stage_active(b.h) == 0
    assert L.vv_ws_epoch() != e0
    shared = frames(a)
    for f, (x, y) in enumerate(zip(solo, shared)):
        e = rel_err(x, y)
        print(f"frame {f}: stage vs launch-per-GEMV audio rel {e:.3e}")
        assert e < 3e-2 and cos(x, y) > 0.999
    e1 = L.vv_ws_epoch()
    b.close()
    assert L.vv_codec_stage_active(a.h) == 1 and L.vv_ws_epoch() != e1
    again = frames(a)
    for x, y in zip(solo, again):
        assert torch.equal(x, y)
    a.close()


@pytest.mark.parametrize("slots_sched", [[[1]] * 4, [[0, 2], [0, 1, 2], [2], [0, 1, 2]]])
def test_codec_tile_narrow_stages(slots_sched):
    """The narrow stages (C = 128 / 64 / 32) as ONE launch each (codec_tile.hip:
    transition conv + 3 Block1Ds [+ head conv], each workgroup recomputing its
    causal halo; 6 launches per codec step instead of 24) vs the oracle and vs
    the launch-per-Block1D path, over four streamed frames -- one sample, and
    several samples with a slot skipping frames (its conv histories must not
    move) -- and bitwise equal run to run.  Both paths are bf16 chains 60+ layers
    deep that sum the transition convs in different orders: the codec tolerance
    (rel L2 < 3e-2, cosine > 0.999) against the oracle and against each other."""
    from vibevoice_amd import _lib
    L = _lib.lib()
    cfg = tiny_config(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    eng = Engine(cfg, sd, dev, max_batch=3, max_ctx=64)
    H = cfg.decoder_config.hidden_size
    dd = ocodec.codec_dims(cfg.acoustic_tokenizer_config, "decoder")
    ed = ocodec.codec_dims(cfg.semantic_tokenizer_config, "encoder")
    sd_a, sd_s = sub(sd, "model.acoustic_tokenizer."), sub(sd, "model.semantic_tokenizer.")
    s_f, b_f = sd["model.speech_scaling_factor"], sd["model.speech_bias_factor"]
    g = torch.Generator().manual_seed(23)
    lats = [torch.randn(len(s), 64, generator=g).bfloat16() for s in slots_sched]
    outs = {}
    try:
        for mode in (1, 0, 1):
            L.vv_codec_tile(mode)
            eng.codec_reset(torch.arange(3, dtype=torch.int32, device=dev))
            res = []
            for slots, lat in zip(slots_sched, lats):
                n = len(slots)
                sl = torch.tensor(slots, dtype=torch.int32, device=dev)
                audio = torch.empty(n, cfg.hop, dtype=torch.bfloat16, device=dev)
                sem = torch.empty(n, 128, dtype=torch.bfloat16, device=dev)
                emb = torch.zeros(3, H, dtype=torch.bfloat16, device=dev)
                eng.codec_step(sl, lat.to(dev), audio, sem, emb, sl)
                res.append((audio, sem, emb[sl.long()]))
            torch.cuda.synchronize()
            outs.setdefault(mode, []).append(res)
    finally:
        L.vv_codec_tile(1)
    eng.check_sync()
    st_a, st_s = ocodec.StreamState(3), ocodec.StreamState(3)
    for f, (slots, lat) in enumerate(zip(slots_sched, lats)):
        idx = torch.tensor(slots)
        a_ref = ocodec.decode(sd_a, dd, (lat / s_f - b_f).unsqueeze(-1), st_a, idx)
        s_ref = ocodec.encode(sd_s, ed, a_ref, st_s, idx)[:, 0]
        e_ref = connector(sd, "model.acoustic_connector.", lat) + connector(sd, "model.semantic_connector.", s_ref)
        for k, (name, ref) in enumerate((("audio", a_ref[:, 0]), ("sem", s_ref), ("emb", e_ref))):
            got, base, again = outs[1][0][f][k], outs[0][0][f][k], outs[1][1][f][k]
            e_o, e_b = rel_err(got, ref), rel_err(got, base)
            print(f"frame {f} slots {slots} {name}: rel {e_o:.3e} vs oracle ({rel_err(base, ref):.3e} per-block "
                  f"path), {e_b:.3e} vs the per-block path")
            assert torch.equal(got, again), (f, name)
            assert e_o < 3e-2 and cos(got, ref) > 0.999, (f, name, e_o)
            assert e_b < 3e-2 and cos(got, base) > 0.999, (f, name, e_b)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_codec_wide_stages(n):
    """The wide stages (C = 256 at T = 200, C = 512 at T = 40; decoder and
    semantic encoder) as ONE launch each (codec_wide.hip: clusters of C / 32
    workgroups per 16-row time tile, each owning 128 hidden units, partials
    reduce-scattered and block outputs all-gathered inside the cluster) vs the
    oracle and vs the k_mix + GEMM path over four streamed frames, n samples
    (their conv histories carried frame to frame), bitwise equal run to run
    (the member order of the partial sums is fixed).  n = 8 (configs[2]) runs
    grids past one resident wave (832 / 384 workgroups; clusters complete in
    dispatch order; vv_codec_wide_over, off by default).  The codec tolerance:
    rel L2 < 3e-2, cosine > 0.999."""
    from vibevoice_amd import _lib
    L = _lib.lib()
    L.vv_codec_wide_over(1 if n > 2 else 0)
    cfg = tiny_config(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    eng = Engine(cfg, sd, dev, max_batch=max(2, n), max_ctx=64)
    active = L.vv_codec_wide_active(eng.h, n)
    if active != 1:
        L.vv_codec_wide_over(0)
    assert active == 1
    H = cfg.decoder_config.hidden_size
    dd = ocodec.codec_dims(cfg.acoustic_tokenizer_config, "decoder")
    ed = ocodec.codec_dims(cfg.semantic_tokenizer_config, "encoder")
    sd_a, sd_s = sub(sd, "model.acoustic_tokenizer."), sub(sd, "model.semantic_tokenizer.")
    s_f, b_f = sd["model.speech_scaling_factor"], sd["model.speech_bias_factor"]
    g = torch.Generator().manual_seed(29 + n)
    lats = [torch.randn(n, 64, generator=g).bfloat16() for _ in range(4)]
    sl = torch.arange(n, dtype=torch.int32, device=dev)
    outs = {}
    try:
        for mode in (1, 0, 1):
            L.vv_codec_wide(mode)
            eng.codec_reset(sl)
            res = []
            for lat in lats:
                audio = torch.empty(n, cfg.hop, dtype=torch.bfloat16, device=dev)
                sem = torch.empty(n, 128, dtype=torch.bfloat16, device=dev)
                emb = torch.zeros(n, H, dtype=torch.bfloat16, device=dev)
                eng.codec_step(sl, lat.to(dev), audio, sem, emb, sl)
                res.append((audio, sem, emb))
            torch.cuda.synchronize()
            outs.setdefault(mode, []).append(res)
    finally:
        L.vv_codec_wide(1)
        L.vv_codec_wide_over(0)
    eng.check_sync()
    assert_counters_consistent(eng)   # a clean run leaves every wait counter at a whole number of waits
    st_a, st_s = ocodec.StreamState(max(2, n)), ocodec.StreamState(max(2, n))
    idx = torch.arange(n)
    for f, lat in enumerate(lats):
        a_ref = ocodec.decode(sd_a, dd, (lat / s_f - b_f).unsqueeze(-1), st_a, idx)
        s_ref = ocodec.encode(sd_s, ed, a_ref, st_s, idx)[:, 0]
        e_ref = connector(sd, "model.acoustic_connector.", lat) + connector(sd, "model.semantic_connector.", s_ref)
        for k, (name, ref) in enumerate((("audio", a_ref[:, 0]), ("sem", s_ref), ("emb", e_ref))):
            got, base, again = outs[1][0][f][k], outs[0][0][f][k], outs[1][1][f][k]
            e_o, e_b = rel_err(got, ref), rel_err(got, base)
            print(f"n={n} frame {f} {name}: rel {e_o:.3e} vs oracle ({rel_err(base, ref):.3e} k_mix + GEMM path), "
                  f"{e_b:.3e} vs that path")
            assert torch.equal(got, again), (f, name)
            assert e_o < 3e-2 and cos(got, ref) > 0.999, (f, name, e_o)
            assert e_b < 3e-2 and cos(got, base) > 0.999, (f, name, e_b)
