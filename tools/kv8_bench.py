"""FP8 (e4m3) KV-cache storage against the bf16 cache, same process, same weights and seed.

  python tools/kv8_bench.py --model 1.5B --batch 1 [--context 65000] [--out profiles/kv8_1.5b_b1.json]
      the decode loop as bench.py times it (a real prefill of the prompt -- with
      --context a script of that many tokens, as bench.py --context builds it --
      warm-up, graph replay, wall clock around K steps after a device
      synchronise), `--repeats` timed blocks per format, bf16 then FP8 KV (one
      engine at a time); reports each block's ms per step, the medians, the engines' KV
      bytes and whether the one-launch attention kernel was on.
      --only bf16 times the bf16 cache alone (runs on a build without the feature
      too: the parent's numbers).
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vibevoice_amd import _lib  # noqa: E402

dev = "cuda"


def main(args):
    from vibevoice_amd.config import VibeVoiceConfig
    from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
    from vibevoice_amd.synthetic import synthetic_inputs, tokenizer_ids
    from vibevoice_amd.weights import synthetic_state_dict
    B, K, Wm, R = args.batch, args.steps, args.warmup, args.repeats
    cfg = VibeVoiceConfig.builtin(args.model)
    sd = synthetic_state_dict(cfg, seed=0, device=dev)
    total = Wm + R * K + 4
    text_tokens = 64
    if args.context:
        mpe = cfg.decoder_config.max_position_embeddings
        args.context = min(args.context, mpe - total - 8)
        base = synthetic_inputs(batch=1, speakers=1, voice_seconds=3.0, text_tokens=0, seed=0)
        text_tokens = max(64, args.context - base["input_ids"].shape[1])
    inp = synthetic_inputs(batch=B, speakers=1, voice_seconds=3.0, text_tokens=text_tokens, seed=100)
    Lp = inp["input_ids"].shape[1]
    tk = tokenizer_ids()
    L = _lib.lib()
    res = dict(model=args.model, batch=B, prompt_tokens=Lp, steps=K, warmup=Wm, repeats=R, ddpm_steps=10)
    formats = [("bf16", None)] + ([] if args.only == "bf16" else [("fp8", "fp8_e4m3")])
    for key, kvd in formats:
        # one engine at a time: two registered contexts on a device switch the one-launch kernels off for both
        kw = {} if kvd is None else {"kv_dtype": kvd}
        model = VibeVoiceForConditionalGenerationInference(cfg, sd, dev, max_batch=B, max_ctx=Lp + total + 8, **kw)
        model.set_ddpm_inference_steps(10)
        torch.manual_seed(1234)
        t0 = time.perf_counter()
        sess = model.generate_session(**inp, tokenizer=tk, cfg_scale=1.3, generation_config={"do_sample": False},
                                      forced_tokens=[[tk.speech_diffusion_id] * total for _ in range(B)],
                                      max_length_times=total / Lp + 1, max_new_tokens=total + 2)
        torch.cuda.synchronize()
        res[key + "_prefill_s"] = round(time.perf_counter() - t0, 3)
        for _ in range(Wm):
            assert sess.step()
        torch.cuda.synchronize()
        if hasattr(model.engine, "kv_bytes"):
            res[key + "_kv_bytes"] = model.engine.kv_bytes()
        res[key + "_lm_attn_active"] = int(L.vv_lm_attn_active(model.engine.h, 2 * B, Lp + Wm))
        blocks = []
        for _ in range(R):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                assert sess.step()
            torch.cuda.synchronize()
            blocks.append(round((time.perf_counter() - t0) / K * 1e3, 4))
        model.engine.check_sync()
        res[key + "_ms_per_step_blocks"] = blocks
        res[key + "_ms_per_step"] = round(statistics.median(blocks), 4)
        print(key, res[key + "_ms_per_step"], "ms/step", blocks, flush=True)
        del sess
        model.engine.close()
        del model
        gc.collect()
        torch.cuda.empty_cache()
    if "fp8_ms_per_step" in res:
        res["fp8_over_bf16"] = round(res["fp8_ms_per_step"] / res["bf16_ms_per_step"], 4)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.5B", choices=["1.5B", "Large"])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--context", type=int, default=0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, choices=[None, "bf16"])
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
