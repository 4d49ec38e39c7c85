"""FP8 (OCP e4m3) KV-cache storage on the GPU (csrc/kv_fp8.hip and the one-byte
instantiations of k_attn / k_attn_pf).

An e4m3 code times a power of two is exact in bf16, and a power of two commutes
with the two roundings attention applies (the bf16 P, the fp32 accumulations),
so an engine with an FP8 cache computes, bit for bit, what the bf16 attention
kernels compute over a bf16 cache holding the dequantised rows.  Hence the
quantiser and the attention kernels are tested bitwise, each on its own, and the
LM pass against the reference with fake-quantised K / V (tests/kv8_ref.py)."""
import ctypes
import gc

import pytest
import torch

import kv8_ref
from attn_ref import head_errs, worst
from gpu_util import rel_err
from oracle import lm as olm
from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.synthetic import tokenizer_ids
from vibevoice_amd.weights import fake_quantize_kv, synthetic_state_dict, write_synthetic_checkpoint

pytestmark = pytest.mark.gpu
dev = "cuda"
I32 = dict(dtype=torch.int32, device=dev)
BF = dict(dtype=torch.bfloat16, device=dev)
TK = tokenizer_ids()
D, E, S, X = TK.speech_diffusion_id, TK.speech_end_id, TK.speech_start_id, TK.eos_token_id
VALID = [151643, 151652, 151653, 151654]
FP8 = "fp8_e4m3"
GQA = [(6, 1), (7, 1)]          # query heads per kv head of VibeVoice-1.5B (12 / 2) and -Large (28 / 4)


@pytest.fixture(autouse=True)
def _collect_engines():
    gc.collect()
    yield


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int16)


def _cfg(heads, kv_heads, layers=2):
    return tiny_config(hidden=128 * heads, layers=layers, heads=heads, kv_heads=kv_heads, inter=256)


def _sd(cfg, seed):
    return synthetic_state_dict(cfg, seed=seed, device="cpu", mode="test", with_acoustic_encoder=False)


def _engine(cfg, sd, kv_dtype, max_batch=2, max_ctx=256, **kw):
    return Engine(cfg, sd, dev, max_batch=max_batch, max_ctx=max_ctx, valid_ids=VALID, kv_dtype=kv_dtype, **kw)


def kv_read(eng, slot, p0, p1):
    nl, nkv = eng.cfg.decoder_config.num_hidden_layers, eng.cfg.decoder_config.num_key_value_heads
    k = torch.empty(nl, nkv, p1 - p0, 128, **BF)
    v = torch.empty_like(k)
    _lib.check(_lib.lib().vv_diag_kv_read(eng.h, slot, p0, p1, P(k), P(v)), "diag_kv_read")
    return k, v


def kv_write(eng, slot, p0, p1, k, v):
    _lib.check(_lib.lib().vv_diag_kv_write(eng.h, slot, p0, p1, P(k.contiguous()), P(v.contiguous())), "diag_kv_write")


# ------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("heads,kv_heads", GQA)
@pytest.mark.parametrize("shape", ["decode", "prefill"])
def test_quantiser_bitwise(heads, kv_heads, shape):
    """Layer 0's cache of an FP8-KV engine == fake_quantize_kv of a bf16 engine's,
    bit for bit (later layers' inputs legitimately differ).  One embedding row is
    zero: with the q|k|v bias the row is not, so the zero row is also written
    directly through the diagnostic write below."""
    cfg = _cfg(heads, kv_heads)
    sd = _sd(cfg, 31)
    H = cfg.decoder_config.hidden_size
    lens = [1, 1, 1] if shape == "decode" else [70, 33]        # prefill: both cross a 32-position V block
    g = torch.Generator().manual_seed(len(lens))
    x = torch.randn(sum(lens), H, generator=g).bfloat16()
    x[0] = 0
    slots = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(n) for n in lens]).to(**I32)
    out_idx = torch.tensor([sum(lens) - 1], **I32)
    got = []
    for kvd in (None, FP8):
        eng = _engine(cfg, sd, kvd, max_batch=2)
        eng.lm_forward(x.to(dev), slots, pos, out_idx)
        torch.cuda.synchronize()
        got.append([kv_read(eng, r, 0, n) for r, n in enumerate(lens)])
        eng.close()
    for r in range(len(lens)):
        for which in (0, 1):
            ref, q = got[0][r][which][0].cpu(), got[1][r][which][0].cpu()     # layer 0
            assert ref.float().abs().max() > 0
            assert torch.equal(bits(q), bits(fake_quantize_kv(ref))), (r, "KV"[which])


def test_kv_write_read_is_fake_quantize():
    """vv_diag_kv_write quantises with the append's quantiser: rows over 2^-12 .. 2^6,
    an all-zero row and a single-element row, across a 32-position block boundary."""
    cfg = _cfg(6, 1)
    eng = _engine(cfg, _sd(cfg, 32), FP8)
    g = torch.Generator().manual_seed(2)
    k = torch.ldexp(torch.randn(2, 1, 40, 128, generator=g), (torch.arange(40) % 19 - 12).reshape(1, 1, 40, 1)).bfloat16()
    v = torch.ldexp(torch.randn(2, 1, 40, 128, generator=g), (torch.arange(40) % 17 - 10).reshape(1, 1, 40, 1)).bfloat16()
    k[0, 0, 3] = 0
    v[1, 0, 35] = 0
    v[1, 0, 35, 7] = -3.0
    kv_write(eng, 1, 20, 60, k.to(dev), v.to(dev))
    kq, vq = kv_read(eng, 1, 20, 60)
    assert torch.equal(bits(kq.cpu()), bits(fake_quantize_kv(k))) and torch.equal(bits(vq.cpu()), bits(fake_quantize_kv(v)))
    assert (kq[0, 0, 3] == 0).all() and torch.equal(vq[1, 0, 35].cpu(), v[1, 0, 35])
    eng.close()


# ------------------------------------------------------------------ 2, 3. attention
@pytest.fixture(scope="module", params=GQA, ids=["G6", "G7"])
def attn_pair(request):
    """(cfg, FP8 engine filled with seeded rows of per-row magnitude 2^-6 .. 2^6, bf16
    engine filled with the FP8 engine's dequantised rows, those rows on the host)."""
    heads, kv_heads = request.param
    cfg = _cfg(heads, kv_heads, layers=1)
    sd = _sd(cfg, 33)
    q8, b16 = _engine(cfg, sd, FP8, max_batch=2), _engine(cfg, sd, None, max_batch=2)
    g = torch.Generator().manual_seed(heads)
    rows = []
    for slot in range(4):
        ex = torch.randint(-6, 7, (1, kv_heads, 256, 1), generator=g)
        k = torch.ldexp(torch.randn(1, kv_heads, 256, 128, generator=g), ex).bfloat16().to(dev)
        v = torch.ldexp(torch.randn(1, kv_heads, 256, 128, generator=g), ex.flip(2)).bfloat16().to(dev)
        kv_write(q8, slot, 0, 256, k, v)
        kd, vd = kv_read(q8, slot, 0, 256)
        kv_write(b16, slot, 0, 256, kd, vd)
        kb, vb = kv_read(b16, slot, 0, 256)
        assert torch.equal(bits(kb), bits(kd)) and torch.equal(bits(vb), bits(vd))
        rows.append((kd[0].float().cpu(), vd[0].float().cpu()))
    yield cfg, q8, b16, rows
    q8.close()
    b16.close()


def _attend(eng, q, slots, pos, form):
    out = torch.full_like(q, float("nan"))
    _lib.check(_lib.lib().vv_diag_attn_ctx(eng.h, 0, q.shape[0], P(q), P(slots), P(pos), form, P(out), stream()),
               "diag_attn_ctx")
    torch.cuda.synchronize()
    return out


def _torch_attention(cfg, rows, q, slots, pos):
    """fp32 attention over the dequantised rows (P rounded to bf16 as the reference's eager path does)."""
    nh, nkv = cfg.decoder_config.num_attention_heads, cfg.decoder_config.num_key_value_heads
    out = []
    for i in range(q.shape[0]):
        k, v = rows[int(slots[i])]
        n = int(pos[i]) + 1
        qi = q[i].float().cpu().view(nh, 128)
        kk = k[:, :n].repeat_interleave(nh // nkv, dim=0)
        vv = v[:, :n].repeat_interleave(nh // nkv, dim=0)
        s = torch.einsum("hd,hnd->hn", qi, kk) * 128 ** -0.5
        p = torch.softmax(s, dim=-1).bfloat16().float()
        out.append(torch.einsum("hn,hnd->hd", p, vv).reshape(-1))
    return torch.stack(out)


def _check_attention(attn_pair, slots_h, pos_h, form, tag):
    cfg, q8, b16, rows = attn_pair
    nh = cfg.decoder_config.num_attention_heads
    g = torch.Generator().manual_seed(len(pos_h) + form)
    q = torch.randn(len(pos_h), nh * 128, generator=g).bfloat16().to(dev)
    slots, pos = torch.tensor(slots_h, **I32), torch.tensor(pos_h, **I32)
    o8, o16 = _attend(q8, q, slots, pos, form), _attend(b16, q, slots, pos, form)
    assert torch.isfinite(o8.float()).all(), tag
    assert torch.equal(bits(o8), bits(o16)), tag                                  # test 2: bitwise
    ref = _torch_attention(cfg, rows, q, slots_h, pos_h)
    e = rel_err(o8.float().cpu(), ref)
    print(f"{tag}: FP8-cache attention vs fp32 torch over the dequantised rows: rel L2 {e:.3e}")
    assert e < 1e-2, (tag, e)                                                     # test 3: tests/test_gpu_lm.py's bound
    eh, i, h = worst(head_errs(o8.float().cpu(), ref.reshape(len(pos_h), nh, 128)))
    print(f"{tag}: worst (row, head) rel L2 {eh:.3e} at row {i} head {h}")
    assert eh < 1e-2, (tag, eh, i, h)                                             # ... per (row, head), not pooled


KEYS = [1, 31, 32, 33, 97, 255]


def test_attention_decode_bitwise(attn_pair):
    # one row per key count (slots cycle), then all of them in one launch
    for n in KEYS:
        _check_attention(attn_pair, [n % 4], [n - 1], 0, f"decode keys={n}")
    _check_attention(attn_pair, [i % 4 for i in range(len(KEYS))], [n - 1 for n in KEYS], 0, "decode ragged")


@pytest.mark.parametrize("form,chunk,merge_in,name", [(0, 32, -1, "in-kernel merge"), (0, 32, 0, "k_attn_merge"),
                                                       (0, 64, -1, "in-kernel merge, 4 waves"),
                                                       (2, 32, -1, "defer"), (2, 128, -1, "defer, 4 waves"),
                                                       (3, 32, -1, "group")])
def test_attention_split_forms_bitwise(attn_pair, form, chunk, merge_in, name):
    L = _lib.lib()
    assert L.vv_attn_tune(chunk, merge_in) == 0
    try:
        # 255 keys: every split active; 97 / 33: fewer active splits than planned; ragged rows in one launch
        _check_attention(attn_pair, [0, 1, 2], [254, 96, 32 if form == 0 else 200], form, f"{name} chunk={chunk}")
    finally:
        L.vv_attn_tune(0, -1)


@pytest.mark.parametrize("nq", [33, 64])
def test_attention_prefill_bitwise(attn_pair, nq):
    L = _lib.lib()
    L.vv_attn_prefill(1)
    try:
        # nq query rows per slot, two slots; the second slot's rows end at key 255
        slots = [0] * nq + [3] * nq
        pos = list(range(nq)) + list(range(256 - nq, 256))
        _check_attention(attn_pair, slots, pos, 1, f"prefill nq={nq} per slot")
    finally:
        L.vv_attn_prefill(-1)


# ------------------------------------------------------------------ 4. vv_kv_copy
def test_kv_copy_fp8():
    cfg = _cfg(6, 1)
    eng = _engine(cfg, _sd(cfg, 34), FP8)
    g = torch.Generator().manual_seed(4)
    ex = torch.randint(-6, 7, (2, 1, 64, 1), generator=g)
    k = torch.ldexp(torch.randn(2, 1, 64, 128, generator=g), ex).bfloat16().to(dev)
    v = torch.ldexp(torch.randn(2, 1, 64, 128, generator=g), ex.flip(2)).bfloat16().to(dev)
    for slot in (0, 2):
        kv_write(eng, slot, 0, 64, k, v)
    before = [kv_read(eng, s, 0, 64) for s in (0, 2)]
    # slot 0: 31 -> 32 (across the 32-position block boundary); slot 2: 40 -> 7
    slots, src, dst = torch.tensor([0, 2], **I32), torch.tensor([31, 40], **I32), torch.tensor([32, 7], **I32)
    _lib.check(_lib.lib().vv_kv_copy(eng.h, 2, P(slots), P(src), P(dst), stream()), "kv_copy")
    torch.cuda.synchronize()
    for i, (s, a, b) in enumerate(((0, 31, 32), (2, 40, 7))):
        kq, vq = kv_read(eng, s, 0, 64)
        assert torch.equal(bits(kq[:, :, b]), bits(before[i][0][:, :, a])) and torch.equal(bits(vq[:, :, b]), bits(before[i][1][:, :, a]))
        keep = [p for p in range(64) if p != b]
        assert torch.equal(bits(kq[:, :, keep]), bits(before[i][0][:, :, keep]))
        assert torch.equal(bits(vq[:, :, keep]), bits(before[i][1][:, :, keep]))
    eng.close()


# ------------------------------------------------------------------ 5. the LM pass
@pytest.mark.parametrize("heads,kv_heads", GQA)
@pytest.mark.parametrize("B", [1, 3])
def test_decode_vs_reference_with_fake_quantised_kv(heads, kv_heads, B):
    """A ragged prefill, then 6 teacher-forced decode steps, against kv8_ref with
    fake_quantize_kv as the hook; the project's fixed per-step bounds (DESIGN.md
    §4: hidden 3e-2, the 4 legal logits 7e-2)."""
    cfg = _cfg(heads, kv_heads)
    sd = _sd(cfg, 35)
    eng = _engine(cfg, sd, FP8, max_batch=4)
    L = _lib.lib()
    assert L.vv_kv_dtype(eng.h) == 1
    assert L.vv_lm_attn_active(eng.h, B, 64) == 0
    pre = "model.language_model."
    osd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    lcfg = dict(cfg.decoder_config)
    H = cfg.decoder_config.hidden_size
    W = sd["lm_head.weight"][VALID].float()
    g = torch.Generator().manual_seed(B)
    lens = [37, 5, 70][:B]
    xs = [torch.randn(n, H, generator=g).bfloat16() for n in lens]
    kvs = [olm.RowKV(lcfg["num_hidden_layers"]) for _ in lens]
    ref = torch.stack([kv8_ref.forward_rows(osd, lcfg, xs[r][None], kvs[r:r + 1], kv_hook=fake_quantize_kv)[0, -1]
                       for r in range(B)])
    slots = torch.cat([torch.full((n,), r) for r, n in enumerate(lens)]).to(**I32)
    pos = torch.cat([torch.arange(n) for n in lens]).to(**I32)
    out_idx = (torch.tensor(lens).cumsum(0) - 1).to(**I32)

    def check(h, logits, ref, tag):
        torch.cuda.synchronize()
        lref = (ref.float() @ W.t()).bfloat16().float()
        eh, el = rel_err(h.float().cpu(), ref.float()), rel_err(logits.cpu(), lref)
        print(f"{tag}: hidden rel {eh:.3e} logits rel {el:.3e}")
        assert eh < 3e-2 and el < 7e-2, (tag, eh, el)

    h, logits = eng.lm_forward(torch.cat(xs).to(dev), slots, pos, out_idx)
    check(h, logits, ref, f"G={heads} B={B} prefill")
    Lp = torch.tensor(lens)
    for s in range(6):
        step_x = torch.randn(B, H, generator=g).bfloat16()
        ref = kv8_ref.forward_rows(osd, lcfg, step_x[:, None], kvs, kv_hook=fake_quantize_kv)[:, -1]
        h, logits = eng.lm_forward(step_x.to(dev), torch.arange(B).to(**I32), Lp.to(**I32), torch.arange(B).to(**I32))
        Lp += 1
        check(h, logits, ref, f"G={heads} B={B} step {s}")
    eng.close()


def test_one_launch_kernels_under_fp8_kv():
    """1.5B layer shapes (where k_lm_attn and k_lm_ffn serve the bf16 engine): under
    FP8 KV the attention half is off, the MLP block stays on."""
    cfg = tiny_config(hidden=1536, layers=1, heads=12, kv_heads=2, inter=8960)
    sd = _sd(cfg, 36)
    L = _lib.lib()
    b = _engine(cfg, sd, None, max_batch=1, max_ctx=256)
    was_attn, was_ffn = L.vv_lm_attn_active(b.h, 2, 64), L.vv_lm_ffn_active(b.h, 2)
    b.close()
    gc.collect()
    q = _engine(cfg, sd, FP8, max_batch=1, max_ctx=256)
    assert L.vv_lm_attn_active(q.h, 2, 64) == 0
    assert L.vv_lm_ffn_active(q.h, 2) == was_ffn == 1
    print("bf16 engine: lm_attn", was_attn, "lm_ffn", was_ffn)
    q.close()


# ------------------------------------------------------------------ 6, 7. the loop
@pytest.fixture(scope="module")
def tiny_kv8():
    cfg = tiny_config()
    m = VibeVoiceForConditionalGenerationInference(cfg, _sd(cfg, 37), dev, max_batch=4, max_ctx=256, kv_dtype=FP8)
    m.set_ddpm_inference_steps(5)
    yield cfg, m
    m.engine.close()


def test_graph_replay_matches_eager_kv8(tiny_kv8):
    cfg, m = tiny_kv8
    assert m.kv_dtype == FP8 and _lib.lib().vv_kv_dtype(m.engine.h) == 1
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 151000, (2, 12), generator=g)
    mask = torch.ones(2, 12, dtype=torch.long)
    sched = [[D] * 3 + [E, S] + [D] * 3 + [X], [D] * 2 + [S] + [D] * 5 + [X]]          # 8 steps
    outs = []
    for graphs in (False, True):
        torch.manual_seed(77)
        outs.append(m.generate(input_ids=ids, attention_mask=mask, tokenizer=TK, cfg_scale=1.3, forced_tokens=sched,
                               use_graphs=graphs, show_progress_bar=False))
    assert len(m._graph_cache) >= 1
    assert torch.equal(outs[0].sequences, outs[1].sequences)
    for b in range(2):
        a0, a1 = outs[0].speech_outputs[b].cpu(), outs[1].speech_outputs[b].cpu()
        assert torch.isfinite(a0.float()).all() and torch.equal(a0, a1)


@pytest.mark.parametrize("weight_dtype", [None, FP8])
def test_from_pretrained_kv_dtype(tmp_path, weight_dtype):
    cfg = tiny_config(hidden=256, layers=2, heads=2, kv_heads=1, inter=512)
    write_synthetic_checkpoint(str(tmp_path), cfg, seed=9, mode="test")
    m = VibeVoiceForConditionalGenerationInference.from_pretrained(str(tmp_path), torch_dtype=torch.bfloat16,
                                                                   device_map="cuda", max_batch=2, max_ctx=128,
                                                                   kv_dtype=FP8, weight_dtype=weight_dtype)
    assert m.kv_dtype == FP8 and m.engine.kv_dtype == FP8 and _lib.lib().vv_kv_dtype(m.engine.h) == 1
    assert m.engine.weights_quantized() == (weight_dtype == FP8)
    m.set_ddpm_inference_steps(3)
    ids = torch.randint(0, 151000, (1, 12), generator=torch.Generator().manual_seed(4))
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        outs.append(m.generate(input_ids=ids, attention_mask=torch.ones(1, 12, dtype=torch.long), tokenizer=TK,
                               cfg_scale=1.3, forced_tokens=[[D, D, D, D, X]], show_progress_bar=False))
    audio = outs[0].speech_outputs[0].float().cpu()
    assert outs[0].sequences.shape == (1, 12 + 5)
    assert audio.shape[-1] == 4 * m.engine.hop and torch.isfinite(audio).all() and audio.abs().max() > 0
    assert torch.equal(outs[0].sequences, outs[1].sequences)
    assert torch.equal(outs[0].speech_outputs[0], outs[1].speech_outputs[0])
    m.engine.close()
    with pytest.raises(ValueError, match="fp8_e4m3"):
        VibeVoiceForConditionalGenerationInference.from_pretrained(str(tmp_path), kv_dtype="int8")


# ------------------------------------------------------------------ 8, 9. capacity, errors, the default
def test_capacity_and_errors():
    cfg = _cfg(6, 1)
    sd = _sd(cfg, 38)
    L = _lib.lib()
    b, q = _engine(cfg, sd, None, max_batch=3, max_ctx=200), _engine(cfg, sd, FP8, max_batch=3, max_ctx=200)
    nb, nq = b.kv_bytes(), q.kv_bytes()
    print(f"KV bytes: bf16 {nb}, fp8 {nq}, ratio {nq / nb:.4f}")
    assert nb > 0 and nq <= 0.52 * nb
    assert L.vv_kv_dtype(q.h) == 1 and L.vv_kv_dtype(b.h) == 0
    assert L.vv_set_kv_dtype(q.h, 0) != 0 and b"after vv_finalize" in L.vv_last_error()
    slots = torch.zeros(1, **I32)
    assert L.vv_kv_synthetic(q.h, 1, P(slots), 0, 8, 1, stream()) != 0 and b"FP8" in L.vv_last_error()
    assert L.vv_kv_synthetic(b.h, 1, P(slots), 0, 8, 1, stream()) == 0
    torch.cuda.synchronize()
    b.close()
    q.close()
    # an unknown dtype, before vv_finalize
    h = ctypes.c_void_p()
    ecfg = q._ecfg
    _lib.check(L.vv_create(ctypes.byref(ecfg), 0, ctypes.byref(h)), "create")
    try:
        assert L.vv_set_kv_dtype(h, 2) != 0 and b"unsupported dtype 2" in L.vv_last_error()
        assert L.vv_set_kv_dtype(h, 1) == 0 and L.vv_kv_dtype(h) == 1
        n = ctypes.c_longlong(-1)
        assert L.vv_kv_bytes(h, ctypes.byref(n)) != 0 and b"before vv_finalize" in L.vv_last_error()
        assert L.vv_tp_init(h, 0, 2, None) != 0 and b"tensor-parallel" in L.vv_last_error()
    finally:
        L.vv_destroy(h)
    # tensor parallelism: refused in Python before anything is built
    with pytest.raises(ValueError, match="tensor parallel"):
        Engine(cfg, sd, dev, max_batch=1, max_ctx=64, tp_rank=0, tp_size=2, kv_dtype=FP8)
    with pytest.raises(ValueError, match="fp8_e4m3"):
        Engine(cfg, sd, dev, max_batch=1, max_ctx=64, kv_dtype="fp8")


def test_default_engine_is_unchanged():
    """kv_dtype=None: a bf16 cache, and the one-launch attention kernel where it ran before."""
    cfg = tiny_config(hidden=1536, layers=1, heads=12, kv_heads=2, inter=8960)
    eng = _engine(cfg, _sd(cfg, 39), None, max_batch=1, max_ctx=256)
    L = _lib.lib()
    assert eng.kv_dtype is None and L.vv_kv_dtype(eng.h) == 0
    assert L.vv_lm_attn_active(eng.h, 2, 64) == 1 and L.vv_lm_ffn_active(eng.h, 2) == 1
    eng.close()
