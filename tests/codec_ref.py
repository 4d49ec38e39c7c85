"""CPU reference of the streaming σ-VAE codec, one stage at a time.  No GPU
imports; tests/test_gpu_codec_stages.py feeds it the engine's own stage inputs
and histories (vv_diag_codec_state) and compares every stage's output and
streaming state with it, and tests/test_codec_ref_cpu.py pins it to
oracle/codec.py.

A stage of the acoustic decoder is the conv before its Block1Ds (the stem for
stage 0, the transposed conv `upsample_layers.i` after it), the Block1Ds, and
for the last stage the head conv.  A stage of the (semantic) encoder is the
same with the strided conv `downsample_layers.i` before the blocks.

`run_stage(..., torch.bfloat16)` is oracle/codec.py's arithmetic op for op (the
chain of all stages equals oracle.codec.decode / encode bit for bit; the
roundings are the ones the header of csrc/codec_block.hip lists):

    n_t   = bf16(bf16(x_t * rsqrt(mean(x_t^2) + eps)) * norm_w)    -> the mixer's conv input and history
    y_t   = x_t + bf16(bf16(dwconv_k7(n)_t + b) * gamma)
    a_t   = ConvRMSNorm_ffn(y_t)
    out_t = y_t + bf16(ffn_gamma * bf16(fc2(bf16(GELU(bf16(fc1(a_t)))))))

`run_stage(..., torch.float64)` is the reference proper: the same bf16 weights,
inputs and histories upcast, no rounding in between.

Tensors are the oracle's: activations [n, C, T], histories {StreamState key:
[n, C, ctx]}.  The engine keeps the same state time-major per slot ([ctx + T
rows][C] per conv buffer); `parse_layout` .. `state_rows` map between the two.
One difference: the decoder's transposed conv has 2 taps per output (k = 2 x
stride), so the engine keeps 1 history row where the oracle keeps k - 1 (only
the last of them reaches an output that is kept).

`mut` mutates the reference for the tests that show a bound has teeth:
    {"block": j, "zero_row": r}     history row r of block j's mixer read as zero
    {"block": j, "tap_shift": 1}    block j's depthwise taps shifted by one
    {"block": j, "swap_gamma": 1}   gamma <-> ffn_gamma in block j
    {"block": j, "gamma_chunk": c}  channels [8c, 8c + 8) of gamma taken from the next chunk
    {"block": j, "roll_early": 1}   block j's new history ends one row early (rows [T-1, T-1+ctx) kept)
"""
import torch
import torch.nn.functional as F

K = 7     # stem / head / mixer kernel


# ------------------------------------------------------------------ names
def net_name(part):
    return "dec" if part == "decoder" else "enc"


def pre_key(part, i):
    """StreamState key of the conv before stage i's blocks."""
    if part == "decoder":
        return "dec.stem" if i == 0 else f"dec.up{i}"
    return f"enc.down{i}"


def mixer_key(part, i, j):
    return f"{part}.stages.{i}.{j}.mixer"


def head_key(part):
    return net_name(part) + ".head"


def stage_keys(part, dims, i):
    keys = [pre_key(part, i)] + [mixer_key(part, i, j) for j in range(dims["depths"][i])]
    if i == len(dims["depths"]) - 1:
        keys.append(head_key(part))
    return keys


def pre_weight(part, i):
    if part == "decoder":
        return "decoder.upsample_layers.0.0.conv.conv." if i == 0 else f"decoder.upsample_layers.{i}.0.convtr.convtr."
    return f"encoder.downsample_layers.{i}.0.conv.conv."


def stage_weights(sd, dims, part, i, dtype):
    """The tensors stage i reads, cast to dtype (run_stage casts on the fly otherwise)."""
    pre = [pre_weight(part, i), f"{part}.stages.{i}."]
    if i == len(dims["depths"]) - 1:
        pre.append(f"{part}.head.conv.conv.")
    return {k: v.to(dtype) for k, v in sd.items() if any(k.startswith(p) for p in pre)}


def hist_ctx(part, dims, key_kind, i):
    """History length (oracle) of the conv before stage i ("pre"), a mixer or the head."""
    if key_kind != "pre" or i == 0:
        return K - 1
    r = dims["ratios"][i - 1]
    return 2 * r - 1 if part == "decoder" else r


def zero_hist(sd, dims, part, i, n, dtype):
    """Zero histories of every conv of stage i (a slot's first frame, or after a reset)."""
    chans = dims["chans"]
    cin = chans[i - 1] if i > 0 else (dims["vae_dim"] if part == "decoder" else dims["channels"])
    h = {pre_key(part, i): torch.zeros(n, cin, hist_ctx(part, dims, "pre", i), dtype=dtype)}
    for j in range(dims["depths"][i]):
        h[mixer_key(part, i, j)] = torch.zeros(n, chans[i], K - 1, dtype=dtype)
    if i == len(chans) - 1:
        h[head_key(part)] = torch.zeros(n, chans[i], K - 1, dtype=dtype)
    return h


# ------------------------------------------------------------------ the stage
def _rms_norm(x, w, eps, acc):
    """ConvRMSNorm on [n, C, T]: normalise in `acc`, cast back, times w (oracle.codec.conv_rms_norm)."""
    y = x.transpose(1, 2)
    o = y.to(acc)
    o = (o * torch.rsqrt(o.pow(2).mean(-1, keepdim=True) + eps)).type_as(y)
    o = o * w
    return o.transpose(1, 2)


def _block(sd, p, x, eps, hist, acc, mut):
    """Block1D with a depthwise mixer -> (out, normalised conv input rows, new history)."""
    dt = x.dtype
    W = lambda k: sd[p + k].to(dt)
    gamma, ffn_gamma = W("gamma"), W("ffn_gamma")
    w, b = W("mixer.conv.conv.conv.weight"), W("mixer.conv.conv.conv.bias")
    if mut.get("swap_gamma"):
        gamma, ffn_gamma = ffn_gamma, gamma
    if "gamma_chunk" in mut:
        c0 = 8 * mut["gamma_chunk"]
        gamma = gamma.clone()
        gamma[c0:c0 + 8] = gamma[c0 + 8:c0 + 16]
    if mut.get("tap_shift"):
        w = torch.roll(w, 1, -1)
    if "zero_row" in mut:
        hist = hist.clone()
        hist[:, :, mut["zero_row"]] = 0
    r = x
    h = _rms_norm(x, W("norm.weight"), eps, acc)
    hin = torch.cat([hist, h], dim=2)
    L = hin.shape[2]
    new_hist = hin[:, :, L - (K - 1) - 1:L - 1] if mut.get("roll_early") else hin[:, :, L - (K - 1):]
    c = F.conv1d(hin, w, b, groups=w.shape[0])
    x = r + c * gamma.unsqueeze(-1)
    r = x
    a = _rms_norm(x, W("ffn_norm.weight"), eps, acc).permute(0, 2, 1)
    f = F.linear(F.gelu(F.linear(a, W("ffn.linear1.weight"), W("ffn.linear1.bias"))),
                 W("ffn.linear2.weight"), W("ffn.linear2.bias")).permute(0, 2, 1)
    return r + f * ffn_gamma.unsqueeze(-1), h, new_hist


def _sconv(x, w, b, stride, hist):
    """Streaming causal conv (oracle.codec.sconv): -> (output, new history)."""
    xin = torch.cat([hist, x], dim=2)
    ctx = hist.shape[2]
    return F.conv1d(xin, w, b, stride=stride), xin[:, :, xin.shape[2] - ctx:]


def _sconvtr(x, w, b, stride, hist):
    """Streaming transposed conv (oracle.codec.sconvtr): -> (output, new history)."""
    k, T = w.shape[-1], x.shape[-1]
    full = torch.cat([hist, x], dim=2)
    y = F.conv_transpose1d(full, w, b, stride=stride)
    y = y[..., : y.shape[-1] - (k - stride)]
    return y[..., y.shape[-1] - T * stride:], full[:, :, full.shape[2] - (k - 1):]


def run_stage(sd, dims, part, i, x_in, hist, dtype, mut=None):
    """Stage i of `part` ("decoder" / "encoder") on x_in [n, C_in, T_in] with the histories `hist`
    ({key: [n, C, ctx]} for stage_keys(part, dims, i)) ->
      {"x":     the last block's output rows [n, C, T] (the next stage's input rows),
       "final": the head conv's output [n, out, T] (last stage only, else None),
       "norm":  per block, its normalised conv input rows [n, C, T],
       "hist":  the new histories}.
    dtype: torch.bfloat16 (the oracle's arithmetic) or torch.float64 (no intermediate rounding)."""
    assert dtype in (torch.bfloat16, torch.float64)
    acc = torch.float32 if dtype == torch.bfloat16 else torch.float64
    mut = mut or {}
    last = i == len(dims["depths"]) - 1
    x = x_in.to(dtype)
    H = {k: hist[k].to(dtype) for k in stage_keys(part, dims, i)}
    new = {}
    q = pre_weight(part, i)
    w, b = sd[q + "weight"].to(dtype), sd[q + "bias"].to(dtype)
    pk = pre_key(part, i)
    if part == "decoder" and i > 0:
        x, new[pk] = _sconvtr(x, w, b, dims["ratios"][i - 1], H[pk])
    else:
        x, new[pk] = _sconv(x, w, b, 1 if i == 0 else dims["ratios"][i - 1], H[pk])
    norms = []
    for j in range(dims["depths"][i]):
        mk = mixer_key(part, i, j)
        x, nrm, new[mk] = _block(sd, f"{part}.stages.{i}.{j}.", x, dims["eps"], H[mk], acc,
                                      mut if mut.get("block") == j else {})
        norms.append(nrm)
    final = None
    if last:
        hk = head_key(part)
        final, new[hk] = _sconv(x, sd[f"{part}.head.conv.conv.weight"].to(dtype),
                                sd[f"{part}.head.conv.conv.bias"].to(dtype), 1, H[hk])
    return {"x": x, "final": final, "norm": norms, "hist": new}


def run_net(sd, dims, part, x_in, hist, dtype, record=None):
    """All stages chained (each fed the previous one's "x") -> the head output [n, out, T]; `hist`
    ({key: [n, C, ctx]} over the whole net) is replaced in place.  record: a list that receives
    (i, stage input, stage histories, result) per stage."""
    x = x_in
    for i in range(len(dims["depths"])):
        h = {k: hist[k] for k in stage_keys(part, dims, i)}
        r = run_stage(sd, dims, part, i, x, h, dtype)
        if record is not None:
            record.append((i, x, h, r))
        hist.update(r["hist"])
        x = r["x"]
    return r["final"]


def zero_net_hist(sd, dims, part, n, dtype):
    h = {}
    for i in range(len(dims["depths"])):
        h.update(zero_hist(sd, dims, part, i, n, dtype))
    return h


# ------------------------------------------------------------------ error measures
# The GPU bound of a stage is M_GPU x e_cpu(stage) in each measure below, e_cpu being noise_floor()'s figure:
# the bf16 stage against the float64 stage on the CPU.  A kernel makes the same roundings as the bf16 stage and
# differs from it only in the order of its fp32 sums (MFMA chunks, split K), so its error against float64 is
# another draw of the same noise; M_GPU covers the spread between two draws, never more than 4.  The per-draw
# measures that are maxima (row, chunk) or cover few values (first) spread most; the pooled ones sum the squares
# over the draws of a stream (3 frames of a sample on the CPU, every checked (slot, frame) of a GPU test) before
# the maximum, so an error that every frame repeats (a wrong gamma chunk, a wrong history tap) stands out of noise
# that does not.
M_GPU = 2.0

MEASURES = ("whole", "row", "chunk", "first", "pchunk", "pfirst")
PER_DRAW = 4


def errs(got, ref):
    """got, ref [C, T] (one sample, one frame) -> (whole, row, chunk, first) in fp64:
      whole: ||got - ref|| / ||ref||
      row:   max over rows t of ||(got - ref)[:, t]|| / rms_t ||ref[:, t]||   (one wrong row cannot hide in T rows)
      chunk: max over 8-channel chunks c of ||(got - ref)[c]|| / rms_c ||ref[c]||  (nor one chunk in C / 8)
      first: ||(got - ref)[:, :6]|| / ||ref[:, :6]||: the rows a history tap reaches (no maximum over T rows,
             so its floor is the whole's, not the row measure's)
    Pool adds, over several draws:
      pchunk: max over chunks c of sqrt(sum_draws ||(got - ref)[c]||^2 / sum_draws ||ref[c]||^2)
      pfirst: sqrt(sum_draws ||(got - ref)[:, :6]||^2 / sum_draws ||ref[:, :6]||^2)"""
    g, r = got.double(), ref.double()
    d = g - r
    C, T = r.shape
    whole = (d.norm() / r.norm()).item()
    row = (d.norm(dim=0) / (r.norm() / T ** 0.5)).max().item()
    nc = max(1, C // 8)
    dc = d.reshape(nc, -1)
    chunk = (dc.norm(dim=1) / (r.norm() / nc ** 0.5)).max().item()
    first = (d[:, :K - 1].norm() / r[:, :K - 1].norm()).item()
    return whole, row, chunk, first


def quantities(res, ref):
    """The compared quantities of a stage: (name, got [n, C, T], ref [n, C, T]).  "out": the head conv's output
    where the stage has one, else the last block's rows; "x": those rows under a head conv (skipped where res has
    none: the decoder's one-launch last stage keeps only their last 6, which "hist.head" holds); "hist.<j>" /
    "hist.head": the new history of block j's mixer / of the head conv, each with a floor of its own."""
    final = ref["final"] is not None
    yield "out", (res["final"] if final else res["x"]), (ref["final"] if final else ref["x"])
    if final and res.get("x") is not None:
        yield "x", res["x"], ref["x"]
    for k in ref["hist"]:
        if k.endswith(".mixer"):
            yield "hist." + k.split(".")[-2], res["hist"][k], ref["hist"][k]
        elif k.endswith(".head"):
            yield "hist.head", res["hist"][k], ref["hist"][k]


def stage_errs(res, ref, n):
    """{quantity: errs()} of a stage, max over the n samples.  res / ref: run_stage results (or a GPU record)."""
    out = {}
    for name, g, r in quantities(res, ref):
        for s in range(n):
            out[name] = tuple(max(a, b) for a, b in zip(out.get(name, (0, 0, 0, 0)), errs(g[s], r[s])))
    return out


class Pool:
    """The pooled measures of one stage over the draws added: {quantity: (pchunk, pfirst)}."""

    def __init__(self):
        self.acc = {}

    def add(self, res, ref, s):
        """Sample s of a stage's result against its reference."""
        for name, g, r in quantities(res, ref):
            g, r = g[s].double(), r[s].double()
            nc = max(1, r.shape[0] // 8)
            d2, r2 = (g - r).pow(2), r.pow(2)
            a = self.acc.setdefault(name, [0.0, 0.0, 0.0, 0.0])
            a[0] = a[0] + d2.reshape(nc, -1).sum(1)
            a[1] = a[1] + r2.reshape(nc, -1).sum(1)
            a[2] += d2[:, :K - 1].sum().item()
            a[3] += r2[:, :K - 1].sum().item()

    def result(self):
        return {k: ((a[0] / a[1].clamp_min(1e-300)).max().item() ** 0.5, (a[2] / max(a[3], 1e-300)) ** 0.5)
                for k, a in self.acc.items()}


def hist_taps(sd, dims, part, i, hist):
    """Per block of stage i, what the history adds to its depthwise conv: conv([hist | 0]) without bias, fp64."""
    out = []
    for j in range(dims["depths"][i]):
        w = sd[f"{part}.stages.{i}.{j}.mixer.conv.conv.conv.weight"].double()
        h = hist[mixer_key(part, i, j)].double()
        out.append(F.conv1d(torch.cat([h, torch.zeros_like(h[:, :, :1])], dim=2), w, None, groups=w.shape[0]))
    return out


def noise_floor(sd_by_part, dims_by_part, lat_frames, scaling, bias, n, w64=None, recs=None):
    """e_cpu: for each (part, stage), the errors of the bfloat16 stage against the float64 stage on identical
    inputs and histories (the bf16 chain's own) over a CPU stream decoder -> encoder: the per-draw measures'
    maximum over the frames and the n samples, the pooled measures per sample over the frames, maximum over the
    samples.  lat_frames: [frames][n, vae] bf16 latents.  -> {(part, stage): {quantity: MEASURES tuple}}.
    w64: a dict that keeps the float64 weights per (part, stage); recs: one that receives the bf16 records."""
    dd, ed = dims_by_part["decoder"], dims_by_part["encoder"]
    hd = zero_net_hist(sd_by_part["decoder"], dd, "decoder", n, torch.bfloat16)
    he = zero_net_hist(sd_by_part["encoder"], ed, "encoder", n, torch.bfloat16)
    recs = {} if recs is None else recs
    recs.update({"decoder": [], "encoder": []})
    for lat in lat_frames:
        z = (lat / scaling - bias).unsqueeze(-1)
        audio = run_net(sd_by_part["decoder"], dd, "decoder", z, hd, torch.bfloat16, recs["decoder"])
        run_net(sd_by_part["encoder"], ed, "encoder", audio, he, torch.bfloat16, recs["encoder"])
    floor = {}
    for part in ("decoder", "encoder"):
        dims, rec = dims_by_part[part], recs[part]
        for i in range(len(dims["depths"])):
            w = stage_weights(sd_by_part[part], dims, part, i, torch.float64)
            if w64 is not None:
                w64[(part, i)] = w
            draw, pools = {}, [Pool() for _ in range(n)]
            for (si, x, h, r) in rec:
                if si != i:
                    continue
                ref = run_stage(w, dims, part, i, x, h, torch.float64)
                for k, v in stage_errs(r, ref, n).items():
                    draw[k] = tuple(max(a, b) for a, b in zip(draw.get(k, (0, 0, 0, 0)), v))
                for s in range(n):
                    pools[s].add(r, ref, s)
            pooled = [p.result() for p in pools]
            floor[(part, i)] = {k: v + tuple(max(p[k][m] for p in pooled) for m in range(2)) for k, v in draw.items()}
    return floor


# ------------------------------------------------------------------ the engine's state dump
KINDS = ("stem", "tr", "mix", "head")


def parse_layout(words):
    """vv_diag_codec_layout's words -> [{kind, stage, block, ctx, T, rows, C, off}] (off: element offset in a dump)."""
    nb = int(words[0])
    out, off = [], 0
    for b in range(nb):
        kind, stage, block, ctx, T, rows, C = (int(v) for v in words[1 + 7 * b: 8 + 7 * b])
        out.append(dict(kind=KINDS[kind], stage=stage, block=block, ctx=ctx, T=T, rows=rows, C=C, off=off))
        off += rows * C
    return out


def layout_elems(layout):
    return layout[-1]["off"] + layout[-1]["rows"] * layout[-1]["C"]


def split_dump(flat, layout):
    """A vv_diag_codec_state dump (1-D) -> one [rows, C] view per buffer."""
    return [flat[b["off"]: b["off"] + b["rows"] * b["C"]].view(b["rows"], b["C"]) for b in layout]


def buf_key(part, b):
    """The StreamState key of a layout entry."""
    if b["kind"] == "stem":
        return pre_key(part, 0)
    if b["kind"] == "tr":
        return pre_key(part, b["stage"])
    if b["kind"] == "mix":
        return mixer_key(part, b["stage"], b["block"])
    return head_key(part)


def find_buf(layout, part, key):
    for n, b in enumerate(layout):
        if buf_key(part, b) == key:
            return n
    raise KeyError(key)


def state_from_rows(rows, part, dims, b):
    """A buffer's history rows [ctx, C] (engine) -> the oracle's [C, ctx_oracle] (the decoder's transposed
    conv: zeros for the k - 2 older inputs the engine does not keep; they reach no kept output)."""
    h = rows.t()
    want = hist_ctx(part, dims, "pre", b["stage"]) if b["kind"] == "tr" else K - 1
    if h.shape[1] < want:
        h = torch.cat([torch.zeros(h.shape[0], want - h.shape[1], dtype=h.dtype), h], dim=1)
    return h.contiguous()


def rows_from_state(t, b):
    """The oracle's [C, ctx_oracle] -> the engine's history rows [ctx, C] (the last ctx inputs)."""
    return t[:, t.shape[1] - b["ctx"]:].t().contiguous()


def hist_from_dumps(bufs_by_sample, layout, part, dims, keys):
    """bufs_by_sample: per sample, split_dump()'s buffers -> {key: [n, C, ctx]} of rows [0, ctx) for `keys`."""
    out = {}
    for k in keys:
        n = find_buf(layout, part, k)
        b = layout[n]
        out[k] = torch.stack([state_from_rows(bufs[n][:b["ctx"]], part, dims, b) for bufs in bufs_by_sample])
    return out


def new_rows(bufs_by_sample, layout, n, T=None):
    """Rows [ctx, ctx + T) of buffer n per sample -> [samples, C, T]."""
    b = layout[n]
    T = b["T"] if T is None else T
    return torch.stack([bufs[n][b["ctx"]: b["ctx"] + T].t() for bufs in bufs_by_sample])


def rolled(pre_buf, post_buf, b):
    """What k_roll must leave in rows [0, ctx): rows [T, T + ctx) of the buffer as it stood before the roll,
    i.e. of [pre-step history | this step's rows] (T < ctx: part of the old history stays)."""
    before = torch.cat([pre_buf[:b["ctx"]], post_buf[b["ctx"]: b["ctx"] + b["T"]]], dim=0)
    return before[b["T"]: b["T"] + b["ctx"]]
