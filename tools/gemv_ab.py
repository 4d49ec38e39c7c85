#!/usr/bin/env python3
"""Bits of the M <= 64 GEMV family on a fixed list of launches, for an A/B of two builds.

    python tools/gemv_ab.py [--lib PATH/libvibevoice_hip.so] [--large] > out.txt

Run it once per build (--lib: another build of the library, e.g. the parent
commit's) and compare the outputs with cmp: every line is a launch's
vv_gemm_plan words (kind, waves, K splits, u, tpw, rw) and sha256[:16] of its
output, so equal files mean equal bits in the same kernel forms.  Inputs come
from CPU generators with fixed seeds.  The list reaches every A-staging
prologue of k_gemv1 (plain / fast, plain / staged, the XF_NORM item form, the
three row-per-wave forms, split-K under both hand-offs, 2 / 4 / 8 tiles per
workgroup and the balanced 5-tile form), k_gemv<2> and k_gemv_w8; the forms only
an engine reaches (q|k|v + o_proj's XF_ATTN_MERGE, the head's adaLN operands,
fc1's XF_MIX) run through one tiny-config engine with the one-launch kernels
off.  XF_SILU_ADD is built but no caller of the library sets it (the head
forms SiLU(cond + t_emb) in k_head_cond and runs a plain GEMM on it), so no
launch can reach it.  --large adds the VibeVoice-Large head (K = 3,584 adaLN
rows: the row-per-wave LDS-DMA form, rw = 2), a 1 GB fixture.
"""
import ctypes
import gc
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from vibevoice_amd import _lib  # noqa: E402

if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])

from tiny import tiny_config  # noqa: E402
from vibevoice_amd.engine import Engine  # noqa: E402
from vibevoice_amd.weights import mfma_pack, mfma_pack8, quantize_rows_e4m3, synthetic_state_dict  # noqa: E402

dev = "cuda"
L = _lib.lib()
CUS = torch.cuda.get_device_properties(0).multi_processor_count


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def sha(*ts):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


def plan(M, N, K, xf, has_w, w8=False, has_mod=False, keep=0):
    out = (ctypes.c_int * 12)()
    fn = L.vv_gemm_plan_w8 if w8 else L.vv_gemm_plan
    _lib.check(fn(M, N, K, xf, int(has_w), int(has_mod), 0, keep, CUS, out, 12 if w8 else 11), "plan")
    words = f"kind {out[0]} waves {out[2]} ks {out[3]} u {out[4]} tpw {out[5]} rw {out[6]}"
    return words + (f" codes {out[11]}" if w8 else "")


def operands(M, N, K):
    g = torch.Generator().manual_seed(1000 * M + N + K)
    A = (2 * torch.randn(M, K, generator=g)).bfloat16()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    nw = (1 + 0.2 * torch.randn(K, generator=g)).bfloat16()
    b = (0.1 * torch.randn(N, generator=g)).bfloat16()
    return A.to(dev), W.to(dev), nw.to(dev), b.to(dev)


def gemm(tag, M, N, K, norm=False, weighted=True):
    A, W, nw, b = operands(M, N, K)
    Y = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if norm:
        _lib.check(L.vv_gemm_bf16_norm(M, N, K, P(A), K, P(nw) if weighted else None, 1e-6, P(mfma_pack(W)),
                                       _lib.EPI["store"], P(Y), N, None, st), tag)
    else:
        _lib.check(L.vv_gemm_bf16(M, N, K, P(A), K, P(mfma_pack(W)), P(b), _lib.EPI["store"], P(Y), N, None, None,
                                  None, st), tag)
    print(f"{tag} M {M} N {N} K {K} | {plan(M, N, K, int(norm), norm and weighted)} | {sha(Y)}", flush=True)


def gemm_w8(tag, M, N, K, norm):
    A, W, nw, b = operands(M, N, K)
    codes, ex = quantize_rows_e4m3(W)
    Y = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cp, ex = mfma_pack8(codes).contiguous(), ex.contiguous()
    _lib.check(L.vv_gemm_w8(M, N, K, P(A), K, P(cp), P(ex), int(norm), P(nw) if norm else None, 1e-6, P(b),
                            _lib.EPI["store"], P(Y), N, None, None, st), tag)
    print(f"{tag} M {M} N {N} K {K} | {plan(M, N, K, int(norm), norm, w8=True)} | {sha(Y)}", flush=True)


def kernel_launches():
    gemm("plain-fast", 2, 256, 1536)
    gemm("plain-staged", 16, 256, 1536)
    L.vv_gemv_tune_rw(99)
    try:
        gemm("norm-item", 2, 256, 1536, norm=True)
        gemm("norm-item", 16, 256, 1536, norm=True)
        gemm("norm-item", 4, 256, 3584, norm=True, weighted=False)
    finally:
        L.vv_gemv_tune_rw(0)
    gemm("norm-rw-ipr3-rpw1", 2, 256, 1536, norm=True)
    L.vv_gemv_tune(8, 0, -1, 0, 0)
    try:
        gemm("norm-rw-ipr3-rpw2", 16, 256, 1536, norm=True)
    finally:
        L.vv_gemv_tune(0, 0, -1, 0, 0)
    gemm("norm-rw-ipr7", 4, 256, 3584, norm=True, weighted=False)
    for h in (0, 1):
        L.vv_gemv_tune(0, 2, h, 0, 0)
        try:
            gemm(f"splitk-handoff{h}", 5, 64, 1536)
            gemm(f"splitk-handoff{h}-norm", 5, 64, 1536, norm=True)
        finally:
            L.vv_gemv_tune(0, 0, -1, 0, 0)
    for tpw in (2, 4, 8):
        L.vv_gemv_tune(8, 0, -1, 0, 0)
        L.vv_gemv_tune_tpw(tpw)
        try:
            gemm(f"tpw{tpw}", 16, 272, 1536)
        finally:
            L.vv_gemv_tune(0, 0, -1, 0, 0)
            L.vv_gemv_tune_tpw(0)
    gemm("tpw5-balanced", 16, 16 * (5 * CUS - 8), 256)
    gemm("k_gemv2", 17, 256, 1536)
    gemm("k_gemv2-norm", 17, 256, 1536, norm=True)
    for M in (2, 16):
        gemm_w8("w8", M, 256, 1536, False)
        gemm_w8("w8-norm", M, 256, 1536, True)


CODEC = dict(ratios=(8, 5, 5, 4, 2, 2), depths="3-3-3-3-3-3-8", nf=32)   # the real codec


def engine_routes(large):
    I32 = dict(dtype=torch.int32, device=dev)
    kw = dict(hidden=3584, heads=28, kv_heads=4, inter=3584, vocab=152064) if large else \
        dict(hidden=1536, heads=12, kv_heads=2, inter=1536, **CODEC)
    tag = "large" if large else "engine"
    H = kw["hidden"]
    cfg = tiny_config(layers=1, **kw)
    sd = synthetic_state_dict(cfg, seed=5, device="cpu", mode="test", with_acoustic_encoder=False)
    eng = Engine(cfg, sd, dev, max_batch=8, max_ctx=1024, persistent=False,
                 valid_ids=[151643, 151652, 151653, 151654])
    g = torch.Generator().manual_seed(23)
    try:
        L.vv_lm_attn(0), L.vv_lm_ffn(0), L.vv_head_m16(0), L.vv_head_fin(0)
        L.vv_codec_stage(0), L.vv_codec_wide(0), L.vv_codec_tile(0)
        if not large:
            # LM decode, 2 rows at 300 keys: q|k|v row-per-wave, o_proj merging 3 deferred key splits (XF_ATTN_MERGE)
            slots = torch.arange(2).to(**I32)
            s = torch.cuda.current_stream()
            _lib.check(L.vv_kv_synthetic(eng.h, 2, P(slots), 0, 300, 7, ctypes.c_void_p(s.cuda_stream)), "kv")
            x = torch.randn(2, H, generator=g).bfloat16().to(dev)
            ap = (ctypes.c_int * 6)()
            _lib.check(L.vv_attn_pass_plan(2, 8, 128, kw["kv_heads"], 301, ap), "attn_pass_plan")
            for step in range(2):
                h, lg = eng.lm_forward(x, slots, torch.full((2,), 300 + step).to(**I32), slots)
                print(f"{tag} lm-decode step {step} | attn nsplit {ap[1]} chunk {ap[2]} defer {ap[3]} | "
                      f"qkv {plan(2, (kw['heads'] + 2 * kw['kv_heads']) * 128, H, 1, True)} | {sha(h)} {sha(lg)}",
                      flush=True)
        # diffusion samples (the adaLN shift / scale operands): n = 1 and 8 rows (2n GEMV rows)
        eng.set_steps(3)
        for n in (1, 8):
            pos, neg = (torch.randn(n, H, generator=g).bfloat16().to(dev) for _ in range(2))
            x = torch.randn(n, 64, generator=g).bfloat16().to(dev)
            eng.diffusion_sample(pos, neg, x, 1.3)
            F = int(H * cfg.diffusion_head_config.head_ffn_ratio)
            # the plan of each layer's gate|up launch (norm weight + adaLN shift / scale operands; the tiny head's
            # weights keep the default cache policy, the Large head's 0.9 GB do not: engine.cpp head_plan)
            print(f"{tag} head n {n} | adaLN gate|up {plan(2 * n, 2 * F, H, 1, True, has_mod=True, keep=int(not large))} | {sha(x)}",
                  flush=True)
        if not large:
            # codec frames at one and two slots: fc1 through k_gemv1's XF_MIX at the T = 1 stage
            for sl in ([1], [0, 2]):
                slots = torch.tensor(sl).to(**I32)
                eng.codec_reset(slots)
                for frame in range(2):
                    lat = torch.randn(len(sl), 64, generator=g).bfloat16().to(dev)
                    audio = torch.empty(len(sl), cfg.hop, dtype=torch.bfloat16, device=dev)
                    sem = torch.empty(len(sl), 128, dtype=torch.bfloat16, device=dev)
                    eng.codec_step(slots, lat, audio, sem)
                    w = (ctypes.c_int * 64)()
                    _lib.check(L.vv_diag_codec_plan(eng.h, 0, len(sl), w, 64), "diag_codec_plan")
                    routes = "".join(str(w[2 + 6 * i]) for i in range(7)) + "x" + "".join(str(w[6 + 6 * i]) for i in range(7))
                    print(f"{tag} codec slots {sl} frame {frame} | dec routes {routes} | {sha(audio)} {sha(sem)}", flush=True)
    finally:
        L.vv_lm_attn(1), L.vv_lm_ffn(1), L.vv_head_m16(1), L.vv_head_fin(1)
        L.vv_codec_stage(1), L.vv_codec_wide(1), L.vv_codec_tile(1)
        eng.close()
        del eng
        gc.collect()


if __name__ == "__main__":
    kernel_launches()
    engine_routes(False)
    if "--large" in sys.argv:
        engine_routes(True)
