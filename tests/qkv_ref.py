"""CPU reference of the LM's q|k|v step: input_layernorm -> q/k/v projection
(+ bias, bf16) -> RoPE on q and k -> the rows the KV cache receives.  No GPU
imports; tests/test_gpu_qkv_append.py compares every kernel form with it.

The arithmetic is the reference model's (HF Qwen2; oracle/lm.py rope_cos_sin /
_rot), with every rounding explicit:

    v     = bf16(acc + bias)                      q/k/v_proj output
    angle = fp32(p) * inv_freq[j]                 fp32, inv_freq by the HF formula
    c, s  = bf16(cos(angle)), bf16(sin(angle))    fp64 cosine / sine of the fp32 angle
    out   = bf16(bf16(v * c) + bf16(rot(v) * s))  q and K;  V = v

Two tiers.  `exact_case` builds inputs whose projection is exact in fp32 in any
summation order (rows of +-1, 1-3 power-of-two weights per output row), so a
kernel must reproduce `exact_ref` bit for bit; `dense_ref` runs seeded random
operands in fp64 and rounds only where the spec rounds.

The one step a CPU cannot reproduce bit for bit is the device's cosf / sinf.
`cos_sin` therefore also returns, per (position, frequency), whether the fp64
cosine or sine lies within relative 2^-20 of a bf16 rounding midpoint; the
output elements rotated by such a value are compared within one bf16 ulp of
max(|v|, |rot v|) instead (`rope_tol`)."""
import torch

D = 128
POS_DECODE = [0, 1, 31, 32, 33, 63, 64, 1000]          # + max_ctx - 1 (decode_positions)
NEAR_REL = 2.0 ** -20


def inv_freq(theta, d=D):
    """Qwen2RotaryEmbedding's default inv_freq (HF modeling_qwen2.py), fp32."""
    return 1.0 / (float(theta) ** (torch.arange(0, d, 2, dtype=torch.int64).to(dtype=torch.float) / d))


def _near_midpoint(x64):
    """|x| within relative NEAR_REL of the midpoint between two adjacent bf16 values."""
    a = x64.abs()
    m, _ = torch.frexp(a)                 # a = m 2^e, m in [0.5, 1): 8 significant bits = m * 256 in [128, 256)
    t = m * 256.0
    frac = t - torch.floor(t)
    return (a > 0) & ((frac - 0.5).abs() <= NEAR_REL * t)


def cos_sin(pos, theta, d=D):
    """pos [n] int -> cos, sin [n, d/2] bf16 and near [n, d/2] bool (see module doc)."""
    ang = pos.to(torch.float32)[:, None] * inv_freq(theta, d)[None, :]      # fp32 product, as the device's
    c64, s64 = ang.double().cos(), ang.double().sin()
    near = _near_midpoint(c64) | _near_midpoint(s64)
    return c64.float().bfloat16(), s64.float().bfloat16(), near


def rot(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def rope(v, cos, sin):
    """v [n, heads, d] bf16 (projection output), cos / sin [n, d/2] bf16 -> bf16(bf16(v c) + bf16(rot(v) s))."""
    assert v.dtype == torch.bfloat16 and cos.dtype == torch.bfloat16
    c = torch.cat([cos, cos], -1)[:, None, :].float()
    s = torch.cat([sin, sin], -1)[:, None, :].float()
    a = (v.float() * c).bfloat16().float()
    b = (rot(v).float() * s).bfloat16().float()
    return (a + b).bfloat16()


def ulp_bf16(x):
    """2^(floor(log2 |x|) - 7); 0 at 0."""
    a = x.double().abs()
    _, e = torch.frexp(a)                 # a in [2^(e-1), 2^e)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 8), torch.zeros_like(a))


def rope_tol(v):
    """ulp_bf16(max(|v|, |rot v|)) per element of v [n, heads, d] (fp64)."""
    return ulp_bf16(torch.maximum(v.double().abs(), rot(v).double().abs()))


def excluded(near, heads):
    """near [n, d/2] -> [n, heads, d]: the output elements that used a near-midpoint cos / sin."""
    return torch.cat([near, near], -1)[:, None, :].expand(-1, heads, -1)


# ------------------------------------------------------------------ operands
def exact_case(H, nh, nkv, seed):
    """Exact-tier operands of one layer: {"norm": [H], "q"/"k"/"v": ([heads*128, H] weight, [heads*128] bias)}.
    norm: bf16 in [0.5, 2).  Each weight row: 1-3 nonzeros +-2^s, |s| <= 3, in different eighths of K (so in
    different 32-wide chunks and different K slices of every kernel).  bias: bf16 with all 8 significant bits
    in use at a magnitude unrelated to the sum's, so acc + bias is rarely a bf16 value."""
    g = torch.Generator().manual_seed(seed)
    norm = (0.5 + 1.5 * torch.rand(H, generator=g)).bfloat16()
    norm = torch.where(norm.float() >= 2.0, torch.full_like(norm, 1.0), norm)
    out = {"norm": norm}

    def draw(N):
        W = torch.zeros(N, H)
        cnt = torch.randint(1, 4, (N,), generator=g)
        eighth = torch.argsort(torch.rand(N, 8, generator=g), dim=1)[:, :3]             # 3 distinct eighths per row
        col = eighth * (H // 8) + torch.randint(0, H // 8, (N, 3), generator=g)
        val = torch.ldexp(torch.where(torch.rand(N, 3, generator=g) < 0.5, -1.0, 1.0),
                          torch.randint(-3, 4, (N, 3), generator=g))
        val = torch.where(torch.arange(3)[None, :] < cnt[:, None], val, torch.zeros(()))
        return W.scatter_(1, col, val)

    heads = (("q", nh), ("k", nkv), ("v", nkv))
    W = draw((nh + 2 * nkv) * D)
    while True:       # no two output rows alike (over q, k and v together): redraw the later one of each pair
        _, inv = torch.unique(W, dim=0, return_inverse=True)
        first = torch.full((int(inv.max()) + 1,), W.shape[0], dtype=torch.long).scatter_reduce(
            0, inv, torch.arange(W.shape[0]), "amin")
        dup = first[inv] != torch.arange(W.shape[0])
        if not bool(dup.any()):
            break
        W[dup] = draw(int(dup.sum()))
    n0 = 0
    for name, h in heads:
        b = (torch.randn(h * D, generator=g) * 0.37).bfloat16()
        out[name] = (W[n0:n0 + h * D].bfloat16().contiguous(), b)
        n0 += h * D
    return out


def sign_rows(n, H, seed):
    """[n, H] bf16 of +-1, another seeded sign pattern per row: mean(x^2) = 1, so the normalised row is +-1."""
    g = torch.Generator().manual_seed(seed)
    return torch.where(torch.rand(n, H, generator=g) < 0.5, -1.0, 1.0).bfloat16()


def dense_case(H, nh, nkv, seed):
    """Dense-tier operands: seeded random bf16 norm weight, fan-in-scaled projections (unit-variance sums), bias.
    q / k bias: 0.1 N(0, 1).  V bias: random sign x U[5, 6).  V's bound is one ulp of the reference value, and an
    fp32 sum of 1,536+ products of magnitude ~1 carries an absolute error near 2^-20 in any order, which is many
    ulps of a value that cancelled to ~2^-15 (8 of 76,800 elements with a 0.1 N(0, 1) bias, fp32 against fp64 on
    the CPU alone); five standard deviations of offset keep |v| >= 2^-4, where one ulp is 2^-12 and the bound
    measures the kernel (dense_ref's callers assert that floor on the reference)."""
    g = torch.Generator().manual_seed(seed)
    out = {"norm": (1.0 + 0.1 * torch.randn(H, generator=g)).bfloat16()}
    for name, heads in (("q", nh), ("k", nkv), ("v", nkv)):
        N = heads * D
        W = (torch.randn(N, H, generator=g) / H ** 0.5).bfloat16()
        if name == "v":
            b = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0) * (5.0 + torch.rand(N, generator=g))
        else:
            b = 0.1 * torch.randn(N, generator=g)
        out[name] = (W, b.bfloat16())
    return out


def state_dict_overrides(case, layer=0):
    """The reference-named tensors of `case` (model.language_model.layers.<layer>.*)."""
    p = f"model.language_model.layers.{layer}."
    sd = {p + "input_layernorm.weight": case["norm"]}
    for n in "qkv":
        sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"] = case[n]
    return sd


# ------------------------------------------------------------------ references
def _finish(proj, pos, theta, nh, nkv):
    """proj: {"q","k","v": [n, heads*128] bf16 projection outputs} -> the result record."""
    n = pos.shape[0]
    cos, sin, near = cos_sin(pos, theta)
    q, k, v = (proj[x].view(n, h, D) for x, h in (("q", nh), ("k", nkv), ("v", nkv)))
    return {"q": rope(q, cos, sin), "k": rope(k, cos, sin), "v": v,
            "q_tol": rope_tol(q), "k_tol": rope_tol(k), "q_excl": excluded(near, nh), "k_excl": excluded(near, nkv)}


def exact_ref(case, x, pos, theta, nh, nkv):
    """x [n, H] of +-1 (sign_rows), pos [n] -> q [n, nh, 128], k / v [n, nkv, 128] bf16 (+ tolerances, exclusions).
    The normalised row is exactly sign * norm; every product and partial sum is exact (checked in fp64)."""
    assert bool((x.float().abs() == 1).all())
    a = x.double() * case["norm"].double()
    proj = {}
    for name in "qkv":
        W, b = case[name]
        acc = a @ W.double().t()
        assert torch.equal(acc.float().double(), acc)                       # exact in fp32
        proj[name] = (acc.float() + b.float()).bfloat16()                   # one fp32 add, one rounding
    return _finish(proj, pos, theta, nh, nkv)


def dense_ref(case, x, pos, theta, nh, nkv, eps):
    """fp64 throughout, bf16 only where the spec rounds: the two norm roundings, the projection output,
    cos / sin, the two products, the sum."""
    xd = x.double()
    xn = (xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)).float().bfloat16()
    a = (case["norm"].double() * xn.double()).float().bfloat16().double()
    proj = {}
    for name in "qkv":
        W, b = case[name]
        proj[name] = (a @ W.double().t() + b.double()).float().bfloat16()
    return _finish(proj, pos, theta, nh, nkv)


# ------------------------------------------------------------------ row layouts
def decode_positions(max_ctx):
    return POS_DECODE + [max_ctx - 1]


def layout_decode(n, max_ctx, first_slot=0):
    """One row per slot: row i in slot first_slot + i at decode_positions[i % 9]."""
    P = decode_positions(max_ctx)
    return [first_slot + i for i in range(n)], [P[i % len(P)] for i in range(n)]


def layout_run(n, start, slot=0):
    return [slot] * n, list(range(start, start + n))


def layout_runs(runs):
    """runs: (slot, start, length) -> concatenated rows."""
    slots, pos = [], []
    for s, p0, n in runs:
        slots += [s] * n
        pos += list(range(p0, p0 + n))
    return slots, pos


def runs_300(max_ctx):
    """Run lengths 137, 45, 3, 115 over slots 0..3: slots change mid-octet (rows 137, 182, 185); the 3-row run
    ends on row 184 (an octet's first row) at position 64 = 0 (mod 8) and slot 3 follows one row later at
    position 65; slot 1's run ends at max_ctx - 1; slot 0's run is octet-aligned from position 0."""
    return layout_runs([(0, 0, 137), (1, max_ctx - 45, 45), (2, 62, 3), (3, 65, 115)])


def permuted(slots, pos, seed):
    perm = torch.randperm(len(pos), generator=torch.Generator().manual_seed(seed)).tolist()
    return [slots[i] for i in perm], [pos[i] for i in perm]
