"""tests/codec_ref.py, the per-stage codec reference of test_gpu_codec_stages.py, on the CPU:

  chain check     run_stage(bfloat16) chained over all stages, three streamed frames, equals
                  oracle.codec.decode / encode bit for bit, outputs and final StreamState (the oracle is pinned
                  to the reference's goldens G4 / G5 by test_oracle_golden.py, so this pins the new file too)
  noise floor     e_cpu(stage): the bfloat16 stage against the float64 stage on identical inputs and histories,
                  for the stage output and the mixer / head histories: what the GPU bound is built from
                  (codec_ref.M_GPU x e_cpu per quantity in each of codec_ref.MEASURES)
  mutation checks a reference with one wrong history row, shifted taps, swapped gammas, a gamma chunk from its
                  neighbour, a stale history or a roll that ends one row early misses the clean float64 run by
                  at least 2 x the GPU bound in the stage it touches, counting only the quantities and measures
                  test_gpu_codec_stages.py asserts: the bound has teeth.  Whole-stage rel L2 alone does not (one
                  history row of a T = 3,200 stage moves it by 1e-3): the row, chunk and first-rows measures, a
                  floor per history buffer and the measures pooled over a stream's frames are what clears
                  (worst: 2.27 x, the gamma chunk in the last block of the encoder's C = 2,048 stage).
"""
import pytest
import torch

import codec_ref as cr
from oracle import codec as ocodec
from tiny import tiny_config
from vibevoice_amd.weights import synthetic_state_dict

FRAMES = 3


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def setup(ratios, depths, n, seed, floor):
    cfg = tiny_config(ratios=ratios, depths=depths, nf=32)
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    S = dict(cfg=cfg, n=n)
    S["sd"] = {"decoder": sub(sd, "model.acoustic_tokenizer."), "encoder": sub(sd, "model.semantic_tokenizer.")}
    S["dims"] = {"decoder": ocodec.codec_dims(cfg.acoustic_tokenizer_config, "decoder"),
                 "encoder": ocodec.codec_dims(cfg.semantic_tokenizer_config, "encoder")}
    S["scale"], S["bias"] = sd["model.speech_scaling_factor"], sd["model.speech_bias_factor"]
    g = torch.Generator().manual_seed(seed)
    S["lats"] = [torch.randn(n, 64, generator=g).bfloat16() for _ in range(FRAMES)]
    if floor:
        S["w64"], S["recs"] = {}, {}
        S["floor"] = cr.noise_floor(S["sd"], S["dims"], S["lats"], S["scale"], S["bias"], n, S["w64"], S["recs"])
    return S


@pytest.fixture(scope="module")
def real():
    """The real codec (ratios 8,5,5,4,2,2; depths 3-3-3-3-3-3-8; 32 filters), n = 2, three frames: the bf16
    chain's per-stage records, the float64 weights per stage and the noise floor."""
    return setup((8, 5, 5, 4, 2, 2), "3-3-3-3-3-3-8", 2, 41, floor=True)


def chain_vs_oracle(S):
    n, sd, dims = S["n"], S["sd"], S["dims"]
    hd = cr.zero_net_hist(sd["decoder"], dims["decoder"], "decoder", n, torch.bfloat16)
    he = cr.zero_net_hist(sd["encoder"], dims["encoder"], "encoder", n, torch.bfloat16)
    st_a, st_s = ocodec.StreamState(n), ocodec.StreamState(n)
    idx = torch.arange(n)
    for f, lat in enumerate(S["lats"]):
        z = (lat / S["scale"] - S["bias"]).unsqueeze(-1)
        audio = cr.run_net(sd["decoder"], dims["decoder"], "decoder", z, hd, torch.bfloat16)
        sem = cr.run_net(sd["encoder"], dims["encoder"], "encoder", audio, he, torch.bfloat16).permute(0, 2, 1)
        a_ref = ocodec.decode(sd["decoder"], dims["decoder"], z, st_a, idx)
        s_ref = ocodec.encode(sd["encoder"], dims["encoder"], a_ref, st_s, idx)
        assert torch.equal(audio, a_ref), ("audio", f)
        assert torch.equal(sem, s_ref), ("sem", f)
    for h, st in ((hd, st_a), (he, st_s)):
        assert set(h) == set(st.buf), set(h) ^ set(st.buf)
        for k in h:
            assert torch.equal(h[k], st.buf[k]), k


def test_chain_equals_oracle_reduced():
    chain_vs_oracle(setup((2, 2), "2-1-2", 3, 43, floor=False))


def test_chain_equals_oracle_real(real):
    chain_vs_oracle(real)


def test_noise_floor(real):
    """Every stage of both nets has a floor in every measure, and it is bf16's: a stage ends in a bf16 rounding
    (rel L2 about 2^-9 / sqrt(3) x 0.7 = 1.6e-3 at the least) and stays within a few dozen roundings of float64."""
    for (part, i), e in sorted(real["floor"].items()):
        for q, (whole, row, chunk, first, pchunk, pfirst) in sorted(e.items()):
            print(f"e_cpu {part} stage {i} {q}: whole {whole:.3e} row {row:.3e} chunk {chunk:.3e} first {first:.3e} "
                  f"pchunk {pchunk:.3e} pfirst {pfirst:.3e}")
            assert 5e-4 < whole < 2e-2 and whole <= chunk and row > 0, (part, i, q)
    for part in ("decoder", "encoder"):
        assert {i for p, i in real["floor"] if p == part} == set(range(7))
        assert all({"out", "hist.0"} <= set(real["floor"][(part, i)]) for i in range(7))


def stage_record(S, part, i, frame):
    return [r for r in S["recs"][part] if r[0] == i][frame]


def asserted_on_gpu(part, dims, i, q):
    """test_gpu_codec_stages.py compares every quantity but the decoder's last block rows (its one-launch last
    stage keeps only their last 6, which the head history holds)."""
    return not (q == "x" and part == "decoder")


def clean_run(S, part, i, frame):
    key = (part, i, frame)
    if key not in S.setdefault("clean", {}):
        _, x, h, _ = stage_record(S, part, i, frame)
        S["clean"][key] = cr.run_stage(S["w64"][(part, i)], S["dims"][part], part, i, x, h, torch.float64)
    return S["clean"][key]


def mutated_run(S, part, i, j, mutation, frame):
    dims = S["dims"][part]
    _, x, h, _ = stage_record(S, part, i, frame)
    mut = {"block": j}
    if mutation == "zero_row":
        mut["zero_row"] = 5 - j % 3
    elif mutation == "gamma_chunk":
        mut["gamma_chunk"] = (j + 1) % (dims["chans"][i] // 8 - 1)
    elif mutation == "stale_hist":
        mut = None
        if frame > 0:
            k = cr.mixer_key(part, i, j)
            h = dict(h)
            h[k] = stage_record(S, part, i, frame - 1)[2][k]
    else:
        mut[mutation] = 1
    return cr.run_stage(S["w64"][(part, i)], dims, part, i, x, h, torch.float64, mut)


def ratio(S, part, i, j, mutation):
    """The mutated float64 run's distance from the clean one over the GPU bound, best over the (quantity,
    measure) pairs the GPU test asserts: the per-draw measures of frame 2, and, where those do not reach 2, the
    pooled measures of a sample's three frames with the mutation in each (as a wrong kernel would have it)."""
    floor, dims = S["floor"][(part, i)], S["dims"][part]
    best = (0.0, "")
    e = cr.stage_errs(mutated_run(S, part, i, j, mutation, 2), clean_run(S, part, i, 2), S["n"])
    for q, v in e.items():
        for m in range(cr.PER_DRAW):
            if asserted_on_gpu(part, dims, i, q):
                best = max(best, (v[m] / (cr.M_GPU * floor[q][m]), f"{q}/{cr.MEASURES[m]}"))
    if best[0] >= 2.0:
        return best
    pools = [cr.Pool() for _ in range(S["n"])]
    for f in range(FRAMES):
        got, clean = mutated_run(S, part, i, j, mutation, f), clean_run(S, part, i, f)
        for s in range(S["n"]):
            pools[s].add(got, clean, s)
    for p in pools:
        for q, v in p.result().items():
            for m in range(2):
                if asserted_on_gpu(part, dims, i, q):
                    k = cr.PER_DRAW + m
                    best = max(best, (v[m] / (cr.M_GPU * floor[q][k]), f"{q}/{cr.MEASURES[k]}"))
    return best


STAGES = [(p, i) for p in ("decoder", "encoder") for i in range(7)]
MUTS = ["zero_row", "tap_shift", "swap_gamma", "gamma_chunk", "stale_hist", "roll_early"]


@pytest.mark.parametrize("mutation", MUTS)
def test_mutation_clears_the_bound(real, mutation):
    """Each mutation, in the first, a middle and the last block of every stage of both nets, is at least 2 x the
    GPU bound away from the clean float64 run, in a quantity and measure the GPU test asserts."""
    S = real
    worst = (1e30, None)
    for part, i in STAGES:
        depth = S["dims"][part]["depths"][i]
        for j in sorted({0, depth // 2, depth - 1}):
            r, where = ratio(S, part, i, j, mutation)
            print(f"{mutation} {part} stage {i} block {j}: {r:.2f} x the bound ({where})")
            worst = min(worst, (r, (part, i, j, where)))
    assert worst[0] >= 2.0, worst


def test_roll_early_at_T1(real):
    """T = 1 < ctx = 6 (the decoder's first stage, the encoder's last): a roll that keeps rows [T-1, T-1+ctx)
    leaves the old history in place; every history row is then one frame stale."""
    S = real
    for part, i in (("decoder", 0), ("encoder", 6)):
        dims = S["dims"][part]
        _, x, h, _ = stage_record(S, part, i, 2)
        assert x.shape[-1] == 1 or part == "encoder"
        w = S["w64"][(part, i)]
        clean = cr.run_stage(w, dims, part, i, x, h, torch.float64)
        got = cr.run_stage(w, dims, part, i, x, h, torch.float64, {"block": 0, "roll_early": 1})
        k = cr.mixer_key(part, i, 0)
        assert clean["norm"][0].shape[-1] == 1
        assert torch.equal(got["hist"][k], h[k].double())            # nothing moved
        assert torch.equal(clean["hist"][k][:, :, :5], h[k].double()[:, :, 1:])
        r, where = ratio(S, part, i, 0, "roll_early")
        print(f"roll_early at T = 1, {part} stage {i}: {r:.1f} x the bound ({where})")
        assert r >= 2.0 and where.startswith("hist.0")


def test_state_layout_round_trip():
    """Engine rows <-> StreamState tensors: transposed, and the decoder's transposed conv keeps 1 of k - 1 inputs."""
    dims = ocodec.codec_dims(tiny_config(ratios=(2, 2), depths="2-1-2", nf=32).acoustic_tokenizer_config, "decoder")
    words = [3, 0, 0, 0, 6, 1, 7, 64, 1, 1, 0, 1, 1, 2, 128, 2, 1, 0, 6, 2, 8, 64]
    lay = cr.parse_layout(words)
    assert [b["off"] for b in lay] == [0, 7 * 64, 7 * 64 + 2 * 128] and cr.layout_elems(lay) == 7 * 64 + 256 + 512
    assert [cr.buf_key("decoder", b) for b in lay] == ["dec.stem", "dec.up1", "decoder.stages.1.0.mixer"]
    assert cr.buf_key("encoder", lay[1]) == "enc.down1" and cr.buf_key("encoder", lay[0]) == "enc.down0"
    flat = torch.arange(cr.layout_elems(lay), dtype=torch.float32)
    bufs = cr.split_dump(flat, lay)
    up = cr.state_from_rows(bufs[1][:1], "decoder", dims, lay[1])        # k = 4: 3 history inputs in the oracle
    assert up.shape == (128, 3) and not up[:, :2].any() and torch.equal(up[:, 2], bufs[1][0])
    assert torch.equal(cr.rows_from_state(up, lay[1]), bufs[1][:1])
    mx = cr.state_from_rows(bufs[2][:6], "decoder", dims, lay[2])
    assert mx.shape == (64, 6) and torch.equal(cr.rows_from_state(mx, lay[2]), bufs[2][:6])
    pre, post = bufs[2].clone(), bufs[2] + 1000
    assert torch.equal(cr.rolled(pre, post, lay[2]), torch.cat([pre[2:6], post[6:8]]))     # T = 2 < ctx = 6
