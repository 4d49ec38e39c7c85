#!/usr/bin/env python
"""Decode step time and attention-half time of a 1.5B engine with an FP8 (e4m3)
KV cache, with the one-launch attention kernel on it (lm_attn.hip's KVQ = 1 form
of k_lm_attn: Engine(lm_attn_kv8=True)), without it (the default: the q|k|v GEMV,
k_kv_quant, k_attn and the o_proj GEMV per layer, k_kv_stage_prep per pass) and
against a bf16 cache -- the A/B behind DESIGN.md "FP8 KV cache".

Step time: bench.py's workload (synthetic 1.5B weights, seed 0, 3 s voice
prompt, 64 text tokens, 10 solver steps, forced diffusion tokens) at B = 1
(2 LM rows) and B = 8 (16 rows); --context N lengthens the text prompt so that
the timed steps end near N keys (N <= 4,096 keeps k_lm_attn on).
Attention-half time: vv_lm_attn_replay over the 28 layers in captured graphs of 1
and 3 passes at the loop's last position (the difference / 56 = one half), as
the engine runs the half, and under vv_lm_attn(0) the launches it replaces.

  one measurement (one JSON line):
    python tools/kv8_lm_attn_bench.py --batch 8 --config kv8_on
  the interleaved A/B (child processes, one engine each, in turn):
    python tools/kv8_lm_attn_bench.py --ab --batch 1 8 --runs 3 --out profiles
    python tools/kv8_lm_attn_bench.py --ab --batch 1 --context 4096 --runs 3 --out profiles
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("kv8_on", "kv8_off", "bf16")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1])
    ap.add_argument("--config", default="kv8_on", choices=CONFIGS)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="1.5B")
    ap.add_argument("--ab", action="store_true", help="interleaved runs of the three configurations")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--context", type=int, default=0, help="keys at the last timed step (0: bench.py's short prompt)")
    ap.add_argument("--out", default=None, help="--ab: directory for kv8_lm_attn_<model>_b<B>[_ctx<N>].json")
    return ap.parse_args()


def half_us(torch, _lib, eng, M, keys):
    """us per attention half at M rows over `keys` keys as lm_attn_half runs it now."""
    L = _lib.lib()
    x = (torch.randn(M, eng.hidden, device="cuda") * 0.5).bfloat16()
    slots = torch.arange(M, device="cuda", dtype=torch.int32)
    pos = torch.full((M,), keys - 1, device="cuda", dtype=torch.int32)
    s = torch.cuda.Stream()
    nl = eng.cfg.decoder_config.num_hidden_layers

    def call(n):
        return L.vv_lm_attn_replay(eng.h, M, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(slots.data_ptr()),
                                   ctypes.c_void_p(pos.data_ptr()), keys, n, ctypes.c_void_p(s.cuda_stream))
    with torch.cuda.stream(s):
        _lib.check(call(1), "lm_attn_replay")
    torch.cuda.synchronize()
    times = []
    for n in (1, 3):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin(capture_error_mode="thread_local")
            call(n)
            g.capture_end()
            g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(8):
                g.replay()
            e1.record(s)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / 8)
    return round((times[1] - times[0]) / (2 * nl), 3)


def measure(args):
    sys.path.insert(0, HERE)
    import torch
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
    kw = dict(bf16={}, kv8_off=dict(kv_dtype="fp8_e4m3"),
              kv8_on=dict(kv_dtype="fp8_e4m3", lm_attn_kv8=True))[args.config]
    model = VibeVoiceForConditionalGenerationInference.from_pretrained(
        f"synthetic:{args.model}", device_map="cuda:0", synthetic_seed=0, max_batch=B, max_ctx=Lp + total + 8, **kw)
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
    model.engine.check_sync()
    L, eng, M, keys = _lib.lib(), model.engine, 2 * B, Lp + W + K
    res = dict(config=args.config, batch=B, steps=K, warmup=W, model=args.model, step_ms=round(dt / K * 1e3, 4),
               kv_dtype=int(L.vv_kv_dtype(eng.h)), lm_attn_kv8=int(L.vv_lm_attn_kv8(eng.h)), keys=keys,
               kv_bytes=eng.kv_bytes(),
               lm_attn_active=int(L.vv_lm_attn_active(eng.h, M, keys)))
    assert res["lm_attn_active"] == (0 if args.config == "kv8_off" else 1), res
    res["half_us"] = half_us(torch, _lib, eng, M, keys)       # as this engine runs the half
    if res["lm_attn_active"]:                                   # ... and the three launches it replaces
        L.vv_lm_attn(0)
        assert L.vv_lm_attn_active(eng.h, M, keys) == 0
        res["three_us"] = half_us(torch, _lib, eng, M, keys)
        L.vv_lm_attn(1)
    eng.check_sync()
    print(json.dumps(res), flush=True)


def child(args, B, config):
    cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(B), "--config", config, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--model", args.model, "--context", str(args.context)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"kv8_lm_attn_bench: {config} B={B} exited {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def ab(args):
    for B in args.batch:
        runs, half, three, active = ({k: [] for k in CONFIGS} for _ in range(4))
        keys = None
        for p in range(args.runs):
            order = CONFIGS[p % 3:] + CONFIGS[:p % 3]          # rotate who goes first
            for k in order:
                r = child(args, B, k)
                runs[k].append(r["step_ms"])
                half[k].append(r["half_us"])
                active[k].append(r["lm_attn_active"])
                keys = r["keys"]
                if "three_us" in r:
                    three[k].append(r["three_us"])
                print(f"B={B} run {p} {k:8s} {r['step_ms']:.4f} ms/step, attention half {r['half_us']:.2f} us "
                      f"(one launch: {r['lm_attn_active']}), three launches {r.get('three_us')}", flush=True)
        med = {k: round(statistics.median(v), 4) for k, v in runs.items()}
        spreads = {k: round(max(v) - min(v), 4) for k, v in runs.items()}
        res = dict(what="decode step time and attention-half time, FP8 (e4m3) KV cache with the one-launch attention "
                        "kernel on it (kv8_on: lm_attn_kv8=True), without it (kv8_off: the default, four launches per "
                        "layer) and a bf16 cache, interleaved child processes (one engine each)",
                   model=args.model, batch=B, keys_at_last_step=keys, lm_rows_per_step=2 * B, steps=args.steps, warmup=args.warmup,
                   runs=args.runs, step_ms_runs=runs, step_ms_median=med, step_ms_spread=spreads,
                   largest_spread_ms=max(spreads.values()), lm_attn_active=active,
                   half_us_runs=half, half_us_median={k: round(statistics.median(v), 3) for k, v in half.items()},
                   three_launches_us_median={k: round(statistics.median(v), 3) for k, v in three.items() if v},
                   kv8_on_vs_off_ms=round(med["kv8_on"] - med["kv8_off"], 4),
                   kv8_on_vs_bf16_ms=round(med["kv8_on"] - med["bf16"], 4))
        res["on_faster_than_off_by_more_than_largest_spread"] = bool(-res["kv8_on_vs_off_ms"] > res["largest_spread_ms"])
        print(json.dumps(res), flush=True)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"kv8_lm_attn_{args.model.lower()}_b{B}" +
                                   (f"_ctx{args.context}" if args.context else "") + ".json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    a = parse()
    ab(a) if a.ab else measure(a)
