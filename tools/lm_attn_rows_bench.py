#!/usr/bin/env python
"""Decode step time and attention-half time of a 1.5B engine at 9 to 16 dialogues (18 to 32
decode rows), with the one-launch attention kernel's second row class (lm_attn.hip MT = 2:
Engine(lm_attn_max_rows=32)) and without it (the default: the q|k|v GEMM, k_attn and the
o_proj GEMM per layer above 16 rows) -- the A/B behind DESIGN.md §3 "k_lm_attn at 17 to 32
rows".  bf16 KV (no FP8-KV form is built above 16 rows).

Step time: bench.py's workload (tools/long_lm_attn_bench.py's `sized` configuration: max_ctx
sized to the run), `off` = the default, `on` = lm_attn_max_rows = 32.  Attention-half time:
vv_lm_attn_replay over the 28 layers (graphs of 1 and 3 passes, the difference / 56) at
--half-rows rows of --half-keys keys, on one engine with the option: as it runs the half (one
launch) and under vv_lm_attn(0) (three launches).

  one measurement:  python tools/lm_attn_rows_bench.py --config on --batch 9
  interleaved A/B:  python tools/lm_attn_rows_bench.py --ab --batch 9 12 16 --runs 3 --out profiles
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
CONFIGS = ("on", "off")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[9])
    ap.add_argument("--config", default="on", choices=CONFIGS + ("half",))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--half-rows", type=int, nargs="*", default=[18, 24, 32])
    ap.add_argument("--half-keys", type=int, default=512)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="--ab: directory for lm_attn_rows_b<B>.json / lm_attn_rows_half.json")
    return ap.parse_args()


def measure_half(args):
    """One engine with the option: us per attention half, one launch against three launches."""
    sys.path.insert(0, HERE)
    import torch
    from kv8_lm_attn_bench import half_us
    from vibevoice_amd import _lib
    from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference

    model = VibeVoiceForConditionalGenerationInference.from_pretrained(
        "synthetic:1.5B", device_map="cuda:0", synthetic_seed=0, max_batch=16, max_ctx=max(1024, args.half_keys + 8),
        lm_attn_max_rows=32)
    L, eng = _lib.lib(), model.engine
    res = dict(config="half", keys=args.half_keys, one_us={}, three_us={})
    for M in args.half_rows:
        assert L.vv_lm_attn_active(eng.h, M, args.half_keys) == 1, M
        res["one_us"][str(M)] = half_us(torch, _lib, eng, M, args.half_keys)
        L.vv_lm_attn(0)
        assert L.vv_lm_attn_active(eng.h, M, args.half_keys) == 0, M
        res["three_us"][str(M)] = half_us(torch, _lib, eng, M, args.half_keys)
        L.vv_lm_attn(1)
    eng.check_sync()
    print(json.dumps(res), flush=True)


def measure(args):
    sys.path.insert(0, HERE)
    import torch
    from vibevoice_amd import _lib
    from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
    from vibevoice_amd.synthetic import synthetic_inputs, tokenizer_ids

    B, K, W = args.batch[0], args.steps, args.warmup
    total = W + K + 4
    inp = synthetic_inputs(batch=B, speakers=1, voice_seconds=3.0, text_tokens=64, seed=100)
    Lp = inp["input_ids"].shape[1]
    kw = dict(lm_attn_max_rows=32) if args.config == "on" else {}
    model = VibeVoiceForConditionalGenerationInference.from_pretrained(
        "synthetic:1.5B", device_map="cuda:0", synthetic_seed=0, max_batch=B, max_ctx=Lp + total + 8, **kw)
    model.set_ddpm_inference_steps(10)
    tk = tokenizer_ids()
    forced = [[tk.speech_diffusion_id] * total for _ in range(B)]
    torch.manual_seed(1234)
    sess = model.generate_session(**inp, tokenizer=tk, cfg_scale=1.3, generation_config={"do_sample": False},
                                  forced_tokens=forced, max_length_times=total / Lp + 1, max_new_tokens=total + 2)
    for _ in range(W):
        assert sess.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        assert sess.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    L, eng = _lib.lib(), model.engine
    eng.check_sync()
    res = dict(config=args.config, batch=B, rows=2 * B, steps=K, warmup=W, max_ctx=eng.max_ctx, keys=Lp + W + K,
               step_ms=round(dt / K * 1e3, 4), lm_attn_max_rows=int(L.vv_lm_attn_max_rows(eng.h)),
               lm_attn_active_as_planned=int(L.vv_lm_attn_active(eng.h, 2 * B, eng.max_ctx)))
    assert res["lm_attn_active_as_planned"] == (1 if kw or 2 * B <= 16 else 0), res
    print(json.dumps(res), flush=True)


def child(args, B, config):
    cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(B), "--config", config, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--half-keys", str(args.half_keys), "--half-rows"] + [str(r) for r in args.half_rows]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"lm_attn_rows_bench: {config} B={B} exited {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def save(args, name, res):
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, name), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def ab(args):
    for B in args.batch:
        rows = {k: [] for k in CONFIGS}
        for p in range(args.runs):
            for k in CONFIGS[p % 2:] + CONFIGS[:p % 2]:          # rotate who goes first
                r = child(args, B, k)
                rows[k].append(r)
                print(f"B={B} run {p} {k:4s} {r['step_ms']:.4f} ms/step at {r['keys']} keys, max_ctx {r['max_ctx']}", flush=True)
        med = {k: round(statistics.median(r["step_ms"] for r in v), 4) for k, v in rows.items()}
        spread = {k: round(max(r["step_ms"] for r in v) - min(r["step_ms"] for r in v), 4) for k, v in rows.items()}
        save(args, f"lm_attn_rows_b{B}.json",
             dict(what="decode step time; on = lm_attn_max_rows = 32 (k_lm_attn's second row class above 16 rows), off = the "
                       "default (three launches above 16 rows); interleaved child processes, one engine each, bf16 KV",
                  batch=B, rows=2 * B, keys_at_last_step=rows["on"][0]["keys"], steps=args.steps, warmup=args.warmup,
                  runs=args.runs, step_ms_runs={k: [r["step_ms"] for r in v] for k, v in rows.items()},
                  step_ms_median=med, step_ms_spread=spread, largest_spread_ms=max(spread.values()),
                  on_minus_off_ms=round(med["on"] - med["off"], 4)))
    if args.half_rows:
        runs = [child(args, 16, "half") for _ in range(args.runs)]
        stat = {}
        for f in ("one_us", "three_us"):
            stat[f + "_median"] = {n: round(statistics.median(r[f][n] for r in runs), 3) for n in runs[0][f]}
            stat[f + "_spread"] = {n: round(max(r[f][n] for r in runs) - min(r[f][n] for r in runs), 3) for n in runs[0][f]}
        save(args, "lm_attn_rows_half.json",
             dict(what="us per attention half (vv_lm_attn_replay, 28 layers) on an engine with lm_attn_max_rows = 32: one = "
                       "k_lm_attn's second row class, three = the q|k|v, k_attn and o_proj launches (vv_lm_attn(0)); fresh "
                       "child processes", keys=args.half_keys, rows=args.half_rows, runs=args.runs,
                  one_us_runs=[r["one_us"] for r in runs], three_us_runs=[r["three_us"] for r in runs], **stat))


if __name__ == "__main__":
    a = parse()
    ab(a) if a.ab else measure_half(a) if a.config == "half" else measure(a)
