"""FP8 (e4m3) weight-only storage against bf16, same process, same weights and seed.

  python tools/w8_bench.py kernels [--out profiles/w8_kernels.json]
      vv_gemm_w8 vs vv_gemm_bf16 / vv_gemm_bf16_norm at the four LM decode
      shapes of VibeVoice-Large and of 1.5B, M = 2 and 16.  Cold cache: the
      weight buffers rotate through > 512 MB (twice the Infinity Cache), the
      launches are captured into one hipGraph and timed with events around
      graph replays.  Reports us, weight bytes and the fraction of 8 TB/s.
  python tools/w8_bench.py steps --model Large --batch 1 [--out profiles/w8_steps_large_b1.json]
      the decode loop as bench.py times it (warm-up, graph replay, wall clock
      around K steps after a device synchronise), bf16 then FP8, ms per step,
      and the engine-held weight bytes of both.
"""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vibevoice_amd import _lib  # noqa: E402
from vibevoice_amd.weights import mfma_pack, mfma_pack8, quantize_rows_e4m3, dequantize_rows  # noqa: E402

dev = "cuda"
PEAK = 8e12
# (name, N, K, xf, epi): q|k|v (norm, store: the RoPE epilogue needs an engine), o_proj (res), gate|up, down
SHAPES = {
    "Large": [("qkv", 4608, 3584, 1, "store"), ("o_proj", 3584, 3584, 0, "res"),
              ("gate_up", 37888, 3584, 1, "silu_mul"), ("down", 3584, 18944, 0, "res")],
    "1.5B": [("qkv", 2048, 1536, 1, "store"), ("o_proj", 1536, 1536, 0, "res"),
             ("gate_up", 17920, 1536, 1, "silu_mul"), ("down", 1536, 8960, 0, "res")],
}


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def time_graph(launch, ncopies, reps=3, iters=5):
    """launch(i) queues one GEMV on copy i; -> us per launch over graph replays."""
    L = _lib.lib()
    for i in range(ncopies):
        launch(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            for i in range(ncopies):
                launch(i)
    g.replay()
    torch.cuda.synchronize()
    best = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / (reps * ncopies))
    del L
    return sorted(best)[len(best) // 2]


def kernels(args):
    L = _lib.lib()
    rows = []
    for model, shapes in SHAPES.items():
        for name, N, K, xf, epi in shapes:
            gen = torch.Generator(device=dev).manual_seed(N + K)
            W = (torch.randn(N, K, device=dev, generator=gen) * 0.02).bfloat16()
            codes, e = quantize_rows_e4m3(W)
            Wd = dequantize_rows(codes, e)
            ncopies = max(2, -(-(640 << 20) // (N * K)))          # FP8 copies span > 512 MB; bf16 twice that
            wb = [mfma_pack(Wd).clone() for _ in range(ncopies)]
            w8 = [mfma_pack8(codes).clone() for _ in range(ncopies)]
            e = e.contiguous()
            del W, Wd, codes
            outN = N // 2 if epi == "silu_mul" else N
            for M in (2, 16):
                A = torch.randn(M, K, device=dev, generator=gen).bfloat16()
                nw = torch.ones(K, device=dev, dtype=torch.bfloat16)
                R = torch.randn(M, outN, device=dev, generator=gen).bfloat16()
                Y = torch.empty(M, outN, device=dev, dtype=torch.bfloat16)
                ek = _lib.EPI[epi]

                def st():
                    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

                def run_bf16(i):
                    if xf:
                        rc = L.vv_gemm_bf16_norm(M, N, K, P(A), K, P(nw), 1e-6, P(wb[i]), ek, P(Y), outN, None, st())
                    else:
                        rc = L.vv_gemm_bf16(M, N, K, P(A), K, P(wb[i]), None, ek, P(Y), outN, P(R), None, None, st())
                    _lib.check(rc, "bf16")

                def run_w8(i):
                    _lib.check(L.vv_gemm_w8(M, N, K, P(A), K, P(w8[i]), P(e), xf, P(nw) if xf else None, 1e-6, None, ek,
                                            P(Y), outN, P(R) if epi == "res" else None, None, st()), "w8")

                t16 = time_graph(run_bf16, ncopies)
                t8 = time_graph(run_w8, ncopies)
                row = dict(model=model, proj=name, M=M, N=N, K=K, xf=xf, epi=epi, copies=ncopies,
                           bf16_us=round(t16, 2), bf16_bytes=2 * N * K, bf16_frac_of_8TBps=round(2 * N * K / (t16 * 1e-6) / PEAK, 3),
                           fp8_us=round(t8, 2), fp8_bytes=N * K + N, fp8_frac_of_8TBps=round((N * K + N) / (t8 * 1e-6) / PEAK, 3),
                           speedup=round(t16 / t8, 3))
                print(json.dumps(row), flush=True)
                rows.append(row)
            del wb, w8
            gc.collect()
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(what="vv_gemm_w8 vs vv_gemm_bf16(_norm), cold cache (rotating weight copies), hipGraph replay, "
                                "median of 5 replays", rows=rows), f, indent=1)


def held_bytes(w):
    seen, n = set(), 0
    for t in w.values():
        if t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            n += t.numel() * t.element_size()
    return n


def steps(args):
    from vibevoice_amd.config import VibeVoiceConfig
    from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
    from vibevoice_amd.synthetic import synthetic_inputs, tokenizer_ids
    from vibevoice_amd.weights import synthetic_state_dict
    B, K, Wm = args.batch, args.steps, args.warmup
    cfg = VibeVoiceConfig.builtin(args.model)
    sd = synthetic_state_dict(cfg, seed=0, device=dev)
    total = Wm + K + 4
    inp = synthetic_inputs(batch=B, speakers=1, voice_seconds=3.0, text_tokens=64, seed=100)
    Lp = inp["input_ids"].shape[1]
    tk = tokenizer_ids()
    res = dict(model=args.model, batch=B, steps=K, warmup=Wm, ddpm_steps=10)
    for wd in (None, "fp8_e4m3"):
        model = VibeVoiceForConditionalGenerationInference(cfg, sd, dev, max_batch=B, max_ctx=Lp + total + 8,
                                                           weight_dtype=wd)
        model.set_ddpm_inference_steps(10)
        torch.manual_seed(1234)
        sess = model.generate_session(**inp, tokenizer=tk, cfg_scale=1.3, generation_config={"do_sample": False},
                                      forced_tokens=[[tk.speech_diffusion_id] * total for _ in range(B)],
                                      max_length_times=total / Lp + 1, max_new_tokens=total + 2)
        for _ in range(Wm):
            assert sess.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            assert sess.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        model.engine.check_sync()
        key = "bf16" if wd is None else "fp8"
        res[key + "_ms_per_step"] = round(dt / K * 1e3, 4)
        res[key + "_weight_bytes"] = held_bytes(model.engine.w)
        print(key, res[key + "_ms_per_step"], "ms/step", res[key + "_weight_bytes"], "bytes", flush=True)
        del sess
        model.engine.close()
        del model
        gc.collect()
        torch.cuda.empty_cache()
    res["fp8_over_bf16"] = round(res["fp8_ms_per_step"] / res["bf16_ms_per_step"], 4)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--out", default=None)
    s = sub.add_parser("steps")
    s.add_argument("--model", default="Large", choices=["1.5B", "Large"])
    s.add_argument("--batch", type=int, default=1)
    s.add_argument("--steps", type=int, default=100)
    s.add_argument("--warmup", type=int, default=10)
    s.add_argument("--out", default=None)
    a = ap.parse_args()
    kernels(a) if a.cmd == "kernels" else steps(a)
