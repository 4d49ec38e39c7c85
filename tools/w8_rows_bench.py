#!/usr/bin/env python
"""Decode step time with FP8 (e4m3) weight-only LM projections against bf16
at batch sizes whose decode passes have more than 16 rows (B = 16: 32 rows,
B = 32: 64 rows), on this tree and, interleaved, on another built tree (the
parent commit) -- the A/B behind DESIGN.md "FP8 weight-only GEMV" and
INTEGRATION.md §2.  bench.py's workload (synthetic 1.5B weights, seed 0, 3 s
voice prompt, 64 text tokens, 10 solver steps, forced diffusion tokens); the
only difference is the weight_dtype option, which bench.py does not have.

  one measurement (one JSON line):
    python tools/w8_rows_bench.py --batch 32 --weights fp8_e4m3 [--root TREE]
  the interleaved A/B (child processes, one engine each, in turn):
    python tools/w8_rows_bench.py --ab --parent TREE --batch 16 32 --pairs 3 --out profiles
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32])
    ap.add_argument("--weights", default="fp8_e4m3", choices=["fp8_e4m3", "bf16"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="1.5B")
    ap.add_argument("--root", default=HERE, help="the built tree whose vibevoice_amd package is measured")
    ap.add_argument("--ab", action="store_true", help="interleaved pairs, this tree and --parent, both weight formats")
    ap.add_argument("--parent", default=None, help="the other built tree of --ab")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None, help="--ab: directory for w8_rows_<model>_b<B>.json")
    return ap.parse_args()


def measure(args):
    sys.path.insert(0, args.root)
    import torch
    from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
    from vibevoice_amd.synthetic import synthetic_inputs, tokenizer_ids

    B, K, W = args.batch[0], args.steps, args.warmup
    total = W + K + 4
    inp = synthetic_inputs(batch=B, speakers=1, voice_seconds=3.0, text_tokens=64, seed=100)
    L = inp["input_ids"].shape[1]
    kw = dict(weight_dtype="fp8_e4m3") if args.weights == "fp8_e4m3" else {}
    model = VibeVoiceForConditionalGenerationInference.from_pretrained(
        f"synthetic:{args.model}", device_map="cuda:0", synthetic_seed=0, max_batch=B, max_ctx=L + total + 8, **kw)
    model.set_ddpm_inference_steps(10)
    tk = tokenizer_ids()
    forced = [[tk.speech_diffusion_id] * total for _ in range(B)]
    torch.manual_seed(1234)
    sess = model.generate_session(**inp, tokenizer=tk, cfg_scale=1.3, generation_config={"do_sample": False},
                                  forced_tokens=forced, max_length_times=total / L + 1, max_new_tokens=total + 2)
    for _ in range(W):
        assert sess.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        assert sess.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    model.engine.check_sync()
    print(json.dumps(dict(weights=args.weights, batch=B, steps=K, warmup=W, model=args.model,
                          step_ms=round(dt / K * 1e3, 4), quantized=bool(model.engine.weights_quantized()))), flush=True)


def child(root, args, B, weights):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--batch", str(B), "--weights", weights,
           "--steps", str(args.steps), "--warmup", str(args.warmup), "--model", args.model]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"w8_rows_bench: {root} {weights} B={B} exited {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])["step_ms"]


def ab(args):
    if not args.parent:
        raise SystemExit("--ab needs --parent TREE")
    trees = dict(this=args.root, parent=os.path.abspath(args.parent))
    for B in args.batch:
        runs = {f"{t}_{w}": [] for t in trees for w in ("fp8_e4m3", "bf16")}
        for p in range(args.pairs):
            for w in ("fp8_e4m3", "bf16"):
                order = ("this", "parent") if p % 2 == 0 else ("parent", "this")   # alternate who goes first
                for t in order:
                    ms = child(trees[t], args, B, w)
                    runs[f"{t}_{w}"].append(ms)
                    print(f"B={B} pair {p} {t:6s} {w:8s} {ms:.4f} ms/step", flush=True)
        med = {k: round(statistics.median(v), 4) for k, v in runs.items()}
        # run-to-run spread: the largest (max - min) of one configuration's repeats
        spread = round(max(max(v) - min(v) for v in runs.values()), 4)
        res = dict(what="decode step time, FP8 (e4m3) weight-only LM projections vs bf16, this tree vs the parent "
                        "commit, interleaved child processes (one engine each)",
                   model=args.model, batch=B, lm_rows_per_step=2 * B, steps=args.steps, warmup=args.warmup,
                   pairs=args.pairs, step_ms_runs=runs, step_ms_median=med, spread_ms=spread,
                   fp8_vs_parent_fp8_ms=round(med["this_fp8_e4m3"] - med["parent_fp8_e4m3"], 4),
                   bf16_vs_parent_bf16_ms=round(med["this_bf16"] - med["parent_bf16"], 4),
                   fp8_vs_bf16_ms=round(med["this_fp8_e4m3"] - med["this_bf16"], 4))
        print(json.dumps(res), flush=True)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"w8_rows_{args.model.lower()}_b{B}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    a = parse()
    ab(a) if a.ab else measure(a)
