#!/usr/bin/env python
"""Decode step time and MLP-block time of a 1.5B engine with FP8 (e4m3)
weight-only LM projections, where the one-launch MLP kernels now run on the
codes (lm_ffn.hip's W8 forms of k_lm_ffn / k_lm_ffn16), against bf16 and
against another built tree (the parent commit, whose FP8 engines run the
k_gemv_w8 pair) -- the A/B behind DESIGN.md "FP8 weight-only GEMV".

Step time: bench.py's workload (synthetic 1.5B weights, seed 0, 3 s voice
prompt, 64 text tokens, 10 solver steps, forced diffusion tokens) at B = 1
(2 LM rows: k_lm_ffn) and B = 8 (16 rows: k_lm_ffn16).
Block time: vv_lm_mlp_replay over the 28 layers in captured graphs of 1 and 3
passes (the difference / 56 = one block; the 28 layers' weights rotate, 1.2 GB
as FP8 and 2.3 GB as bf16, so every launch reads cold weights): the one-launch
form, and on this tree under vv_lm_ffn_w8(0) / vv_lm_ffn(0) the GEMV pair.

  one measurement (one JSON line):
    python tools/w8_lm_ffn_bench.py --batch 8 --weights fp8_e4m3 [--root TREE]
  the interleaved A/B (child processes, one engine each, in turn):
    python tools/w8_lm_ffn_bench.py --ab --parent TREE --batch 1 8 --pairs 3 --out profiles
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


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1])
    ap.add_argument("--weights", default="fp8_e4m3", choices=["fp8_e4m3", "bf16"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="1.5B")
    ap.add_argument("--root", default=HERE, help="the built tree whose vibevoice_amd package is measured")
    ap.add_argument("--ab", action="store_true", help="interleaved runs, this tree and --parent, both weight formats")
    ap.add_argument("--parent", default=None, help="the other built tree of --ab")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None, help="--ab: directory for w8_lm_ffn_<model>_b<B>.json")
    return ap.parse_args()


def block_us(torch, _lib, eng, M):
    """us per MLP block at M rows as lm_mlp_half runs it now (cold weights)."""
    L = _lib.lib()
    x = (torch.randn(M, 1536, device="cuda") * 0.5).bfloat16()
    act = torch.empty(M, 8960, device="cuda", dtype=torch.bfloat16)
    s = torch.cuda.Stream()
    nl = eng.cfg.decoder_config.num_hidden_layers

    def call(n):
        return L.vv_lm_mlp_replay(eng.h, M, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(act.data_ptr()), n,
                                  ctypes.c_void_p(s.cuda_stream))
    with torch.cuda.stream(s):
        _lib.check(call(1), "lm_mlp_replay")
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
    sys.path.insert(0, args.root)
    import torch
    from vibevoice_amd import _lib
    from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
    from vibevoice_amd.synthetic import synthetic_inputs, tokenizer_ids

    B, K, W = args.batch[0], args.steps, args.warmup
    total = W + K + 4
    inp = synthetic_inputs(batch=B, speakers=1, voice_seconds=3.0, text_tokens=64, seed=100)
    Lp = inp["input_ids"].shape[1]
    kw = dict(weight_dtype="fp8_e4m3") if args.weights == "fp8_e4m3" else {}
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
    L, eng, M = _lib.lib(), model.engine, 2 * B
    res = dict(weights=args.weights, batch=B, steps=K, warmup=W, model=args.model, step_ms=round(dt / K * 1e3, 4),
               quantized=bool(eng.weights_quantized()), lm_ffn_active=int(L.vv_lm_ffn_active(eng.h, M)))
    res["block_us"] = block_us(torch, _lib, eng, M)        # as this tree runs the block by default
    if res["lm_ffn_active"]:                                  # ... and the GEMV pair it replaces
        if hasattr(L, "vv_lm_ffn_w8") and res["quantized"]:
            L.vv_lm_ffn_w8(0)
        else:
            L.vv_lm_ffn(0)
        assert L.vv_lm_ffn_active(eng.h, M) == 0
        res["pair_us"] = block_us(torch, _lib, eng, M)
    eng.check_sync()
    print(json.dumps(res), flush=True)


def child(root, args, B, weights):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--batch", str(B), "--weights", weights,
           "--steps", str(args.steps), "--warmup", str(args.warmup), "--model", args.model]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"w8_lm_ffn_bench: {root} {weights} B={B} exited {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def ab(args):
    if not args.parent:
        raise SystemExit("--ab needs --parent TREE")
    trees = dict(this=args.root, parent=os.path.abspath(args.parent))
    for B in args.batch:
        keys = [f"{t}_{w}" for t in trees for w in ("fp8_e4m3", "bf16")]
        runs, block, pair, active = ({k: [] for k in keys} for _ in range(4))
        for p in range(args.pairs):
            for w in ("fp8_e4m3", "bf16"):
                order = ("this", "parent") if p % 2 == 0 else ("parent", "this")   # alternate who goes first
                for t in order:
                    r = child(trees[t], args, B, w)
                    k = f"{t}_{w}"
                    runs[k].append(r["step_ms"])
                    block[k].append(r["block_us"])
                    active[k].append(r["lm_ffn_active"])
                    if "pair_us" in r:
                        pair[k].append(r["pair_us"])
                    print(f"B={B} run {p} {t:6s} {w:8s} {r['step_ms']:.4f} ms/step, block {r['block_us']:.2f} us "
                          f"(one launch: {r['lm_ffn_active']}), pair {r.get('pair_us')}", flush=True)
        med = {k: round(statistics.median(v), 4) for k, v in runs.items()}
        spreads = {k: round(max(v) - min(v), 4) for k, v in runs.items()}
        res = dict(what="decode step time and MLP-block time, FP8 (e4m3) weight-only LM projections vs bf16, this "
                        "tree (one-launch MLP kernels on the codes) vs the parent commit (k_gemv_w8 pair), "
                        "interleaved child processes (one engine each)",
                   model=args.model, batch=B, lm_rows_per_step=2 * B, steps=args.steps, warmup=args.warmup,
                   pairs=args.pairs, step_ms_runs=runs, step_ms_median=med, step_ms_spread=spreads,
                   lm_ffn_active=active,
                   block_us_median={k: round(statistics.median(v), 3) for k, v in block.items()},
                   gemv_pair_us_median={k: round(statistics.median(v), 3) for k, v in pair.items() if v},
                   fp8_vs_parent_fp8_ms=round(med["this_fp8_e4m3"] - med["parent_fp8_e4m3"], 4),
                   bf16_vs_parent_bf16_ms=round(med["this_bf16"] - med["parent_bf16"], 4),
                   fp8_vs_bf16_ms=round(med["this_fp8_e4m3"] - med["this_bf16"], 4))
        print(json.dumps(res), flush=True)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"w8_lm_ffn_{args.model.lower()}_b{B}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    a = parse()
    ab(a) if a.ab else measure(a)
