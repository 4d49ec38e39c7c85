#!/usr/bin/env python
"""Decode step time and attention-half time of a 1.5B engine whose captured graphs are
planned past 4,096 keys, with the one-launch attention kernel's long form
(lm_attn.hip LONG: Engine(lm_attn_max_keys=max_ctx)) and without it (the default: the
q|k|v GEMV, k_attn and the o_proj GEMV per layer) -- the A/B behind DESIGN.md §3
"k_lm_attn past 4,096 keys".  bf16 KV (the long form reads a bf16 cache).

Configurations: `sized` = max_ctx sized to the run as bench.py sizes it (the short
form whenever the run stays under 4,096 keys), `off` = --max-ctx with the default
option, `on` = --max-ctx with lm_attn_max_keys = max_ctx.
Step time: tools/kv8_lm_attn_bench.py's workload; --context N lengthens the prompt so
the timed steps end near N keys.  Attention-half time: vv_lm_attn_replay over the 28
layers (graphs of 1 and 3 passes, the difference / 56) planned at --half-keys, as
the engine runs the half and under vv_lm_attn(0).

  one measurement:  python tools/long_lm_attn_bench.py --config on --max-ctx 8192
  interleaved A/B:  python tools/long_lm_attn_bench.py --ab --batch 1 8 --max-ctx 8192 --runs 3 --out profiles
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
CONFIGS = ("on", "off", "sized")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1])
    ap.add_argument("--config", default="on", choices=CONFIGS)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--max-ctx", type=int, default=8192)
    ap.add_argument("--context", type=int, default=0, help="keys at the last timed step (0: bench.py's short prompt)")
    ap.add_argument("--half-keys", type=int, nargs="*", default=[], help="also time the attention half planned at these key counts")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="--ab: directory for long_lm_attn_b<B>_max<M>[_ctx<N>].json")
    return ap.parse_args()


def measure(args):
    sys.path.insert(0, HERE)
    import torch
    from kv8_lm_attn_bench import half_us
    from vibevoice_amd import _lib
    from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
    from vibevoice_amd.synthetic import synthetic_inputs, tokenizer_ids

    B, K, W = args.batch[0], args.steps, args.warmup
    total = W + K + 4
    text_tokens = 64
    if args.context:
        base = synthetic_inputs(batch=1, speakers=1, voice_seconds=3.0, text_tokens=0, seed=100)
        text_tokens = max(64, args.context - total - 8 - base["input_ids"].shape[1])
    inp = synthetic_inputs(batch=B, speakers=1, voice_seconds=3.0, text_tokens=text_tokens, seed=100)
    Lp = inp["input_ids"].shape[1]
    max_ctx = Lp + total + 8 if args.config == "sized" else args.max_ctx
    assert Lp + total + 8 <= max_ctx, (Lp, total, max_ctx)
    kw = dict(lm_attn_max_keys=max_ctx) if args.config == "on" and max_ctx > 4096 else {}
    model = VibeVoiceForConditionalGenerationInference.from_pretrained(
        "synthetic:1.5B", device_map="cuda:0", synthetic_seed=0, max_batch=B, max_ctx=max_ctx, **kw)
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
    L, eng, M = _lib.lib(), model.engine, 2 * B
    eng.check_sync()
    res = dict(config=args.config, batch=B, steps=K, warmup=W, max_ctx=eng.max_ctx, keys=Lp + W + K,
               step_ms=round(dt / K * 1e3, 4), lm_attn_max_keys=int(L.vv_lm_attn_max_keys(eng.h)),
               lm_attn_active_as_planned=int(L.vv_lm_attn_active(eng.h, M, eng.max_ctx)), half_us={}, three_us={})
    assert res["lm_attn_active_as_planned"] == (1 if max_ctx <= 4096 or "lm_attn_max_keys" in kw else 0), res
    for keys in args.half_keys:
        if keys > eng.max_ctx:
            continue
        res["half_us"][str(keys)] = half_us(torch, _lib, eng, M, keys)       # as this engine runs the half
        L.vv_lm_attn(0)
        res["three_us"][str(keys)] = half_us(torch, _lib, eng, M, keys)      # the three launches
        L.vv_lm_attn(1)
    eng.check_sync()
    print(json.dumps(res), flush=True)


def child(args, B, config):
    cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(B), "--config", config, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--max-ctx", str(args.max_ctx), "--context", str(args.context),
           "--half-keys"] + [str(k) for k in args.half_keys]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"long_lm_attn_bench: {config} B={B} exited {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def ab(args):
    for B in args.batch:
        rows = {k: [] for k in CONFIGS}
        for p in range(args.runs):
            for k in CONFIGS[p % 3:] + CONFIGS[:p % 3]:          # rotate who goes first
                r = child(args, B, k)
                rows[k].append(r)
                print(f"B={B} run {p} {k:6s} {r['step_ms']:.4f} ms/step at {r['keys']} keys, max_ctx {r['max_ctx']}, "
                      f"half {r['half_us']} three {r['three_us']}", flush=True)
        med = {k: round(statistics.median(r["step_ms"] for r in v), 4) for k, v in rows.items()}
        spread = {k: round(max(r["step_ms"] for r in v) - min(r["step_ms"] for r in v), 4) for k, v in rows.items()}

        def hmed(k, f):
            return {n: round(statistics.median(r[f][n] for r in rows[k]), 3) for n in rows[k][0][f]}
        res = dict(what="decode step time and attention-half time; on = lm_attn_max_keys = max_ctx (k_lm_attn's long form for "
                        "passes planned past 4,096 keys), off = the default (three launches), sized = max_ctx sized to the run; "
                        "interleaved child processes, one engine each, bf16 KV",
                   batch=B, max_ctx=args.max_ctx, keys_at_last_step=rows["on"][0]["keys"], steps=args.steps, warmup=args.warmup,
                   runs=args.runs, step_ms_runs={k: [r["step_ms"] for r in v] for k, v in rows.items()},
                   step_ms_median=med, step_ms_spread=spread, largest_spread_ms=max(spread.values()),
                   on_minus_off_ms=round(med["on"] - med["off"], 4), on_minus_sized_ms=round(med["on"] - med["sized"], 4),
                   half_us_median_on=hmed("on", "half_us"), three_launches_us_median_on=hmed("on", "three_us"))
        print(json.dumps(res), flush=True)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            name = f"long_lm_attn_b{B}_max{args.max_ctx}" + (f"_ctx{args.context}" if args.context else "") + ".json"
            with open(os.path.join(args.out, name), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    a = parse()
    ab(a) if a.ab else measure(a)
