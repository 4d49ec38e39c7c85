"""The attention kernels' reference and the cases that judge them (k_attn, its three merges and k_attn_pf,
csrc/attention.hip).  No GPU code is imported here: tests/test_attn_edges_cpu.py checks, from the
reference alone, that every case below can tell a wrong kernel from a right one, and
tests/test_gpu_attention_edges.py runs the same cases on the device.

Every bound is on the maximum over (row, head) of the rel-L2 error (head_errs), never on a norm pooled
over a launch: a row of L random keys has an output norm of about sqrt(e / L), so a pooled norm is the
short rows' and a long row may be anything.

Cases.  A planted key e of kv head kh has K = 2 sqrt(128) u with u a random unit vector and V = +-24; a
(row, head) aimed at it has q = 15 u + 0.5 randn, a score of 30 against O(1) for the 0.25 randn rest, so
that key is the row's output and a kernel that drops it -- or takes it in from past the row's last key,
where the reference ignores it -- is off by about 1, a hundred times the bound.  A staircase plants one
key per 32-key step with scores rising or falling by a fixed number of nats, so the running max, the
carried alpha and the merge weights e^{m_s - M} take non-trivial values."""
import functools
import math

import torch

HD = 128
BOUND = 1e-2                 # max over (row, head) of the rel-L2 error against attention_ref


def _r32(n):
    return (n + 31) // 32 * 32


# ------------------------------------------------------------------ the reference
def _rows(q, slots, pos, nh):
    q = q.reshape(len(pos), nh, HD)
    return q, [int(s) for s in slots], [int(p) for p in pos]


def _key_index(i, h, n, zero, include):
    z = int(zero[i][h]) if zero is not None else -1
    e = int(include[i][h]) if include is not None else -1
    return (z if 0 <= z < n else -1), (e if e >= n else -1)


def attention_ref(q, K, V, slots, pos, nh, nkv, zero=None, include=None):
    """softmax(q k^T / sqrt(128)) v in fp64 with GQA over keys [0, pos] of the row's slot, no rounding of
    P -> [nq, nh, 128].  q [nq, nh * 128]; K, V [slot][kv head][ctx][128].  zero / include ([nq][nh] key
    indices, -1 for none) are the case checks' what-ifs: that key of the row's range replaced by a zero
    K and V row, or one key from past the row's last taken in as well."""
    q, slots, pos = _rows(q, slots, pos, nh)
    G = nh // nkv
    Kd, Vd = K.double(), V.double()
    out = torch.empty(len(pos), nh, HD, dtype=torch.float64)
    for i, (s, p) in enumerate(zip(slots, pos)):
        n = p + 1
        for kh in range(nkv):
            hs = slice(kh * G, (kh + 1) * G)
            k, v = Kd[s, kh, :n], Vd[s, kh, :n]
            sc = q[i, hs].double() @ k.t() / math.sqrt(HD)            # [G, n]
            ve = None
            for j in range(G):
                z, e = _key_index(i, kh * G + j, n, zero, include)
                if z >= 0:
                    sc[j, z] = 0.0
                if e >= 0:
                    assert ve is None or ve[0] == e
                    ve = (e, j)
            if ve is not None:       # (an included key is the same for every head that includes one)
                e = ve[0]
                se = q[i, hs].double() @ Kd[s, kh, e] / math.sqrt(HD)
                for j in range(G):
                    if _key_index(i, kh * G + j, n, zero, include)[1] < 0:
                        se[j] = -math.inf
                sc = torch.cat([sc, se[:, None]], 1)
                v = torch.cat([v, Vd[s, kh, e][None]], 0)
            pr = torch.softmax(sc, -1)
            o = pr @ v
            for j in range(G):
                z, _ = _key_index(i, kh * G + j, n, zero, include)
                if z >= 0:
                    o[j] -= pr[j, z] * v[z]
            out[i, hs] = o
    return out


def attention_emulated(q, K, V, slots, pos, nh, nkv):
    """The same with the kernels' declared roundings: fp32 scores, P rounded to bf16, l from the unrounded
    P, the output rounded to bf16.  It shows that a case's inputs, not the kernel, stay inside the bound."""
    q, slots, pos = _rows(q, slots, pos, nh)
    G = nh // nkv
    Kf, Vf = K.float(), V.float()
    out = torch.empty(len(pos), nh, HD, dtype=torch.float64)
    for i, (s, p) in enumerate(zip(slots, pos)):
        n = p + 1
        for kh in range(nkv):
            hs = slice(kh * G, (kh + 1) * G)
            sc = (q[i, hs].float() @ Kf[s, kh, :n].t()) * (1.0 / math.sqrt(HD))
            pr = torch.exp(sc - sc.max(-1, keepdim=True).values)
            o = (pr.bfloat16().float() @ Vf[s, kh, :n]) / pr.sum(-1, keepdim=True)
            out[i, hs] = o.bfloat16().double()
    return out


def head_errs(out, ref):
    """rel-L2 of every (row, head) on its own -> [nq, nh]."""
    ref = ref.double().cpu()
    out = out.double().cpu().reshape(ref.shape)
    return (out - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)


def worst(errs):
    """(max, row, head) of a head_errs table; a NaN anywhere is the worst."""
    e = torch.nan_to_num(errs, nan=math.inf)
    i = int(e.argmax())
    return float(e.reshape(-1)[i]), i // e.shape[1], i % e.shape[1]


def pooled_err(out, ref):
    ref = ref.double().cpu()
    out = out.double().cpu().reshape(ref.shape)
    return float((out - ref).norm() / ref.norm())


# ------------------------------------------------------------------ k_attn's split plan, restated
def row_splits(length, nsplit, chunk, group=0):
    """attn_dev.h attn_row_splits -> (the row's split size, active splits, partials)."""
    c = _r32(-(-length // nsplit))
    ch = max(chunk, c)
    nact = -(-length // ch)
    return ch, nact, (-(-nact // group) if group else nact)


def plan_nsplit(max_len, chunk):
    """attention.hip attn_plan for max_len keys (no plan here reaches its 256-split cap)."""
    ns = max(1, -(-max_len // chunk))
    assert ns <= 256
    return ns


def plan_waves(chunk):
    return 8 if chunk >= 256 else 4 if chunk >= 128 else 2


def split_edges(length, nsplit, chunk, nw):
    """The key indices at which k_attn's work changes hands for a row of `length` keys: the first and last
    key of every active split, of every wave's sub-range (per = roundup32(ceil((k1 - k0) / NW))), of every
    32-key step inside a wave and of the two 64-key register sets (c0 + 32, c0 + 64), key 0 and the last."""
    ch, nact, _ = row_splits(length, nsplit, chunk)
    edges = {0, length - 1}
    for s in range(nact):
        k0 = s * ch
        k1 = min(length, k0 + ch)
        edges |= {k0, k1 - 1}
        per = _r32(-(-(k1 - k0) // nw))
        for w in range(nw):
            w0 = k0 + w * per
            w1 = min(k1, w0 + per)
            if w0 >= w1:
                continue
            edges |= {w0, w1 - 1}
            for c0 in range(w0, w1, 32):                       # every 32-key step
                edges |= {c0, min(c0 + 31, w1 - 1)}
            for c0 in range(w0, w1, 64):                       # set A: [c0, c0 + 32), set B: [c0 + 32, c0 + 64)
                edges |= {e for e in (c0 + 31, c0 + 32, c0 + 63, c0 + 64) if e < w1}
    return sorted(edges)


# ------------------------------------------------------------------ cases
class Case:
    """One launch's inputs: q [nq, nh * 128], K / V [slot][kv head][ctx][128] (bf16), slots, pos, and per
    (row, head) the key it is aimed at (-1: none; a key past pos: one the row must not see)."""

    def __init__(self, tag, nh, nkv, q, K, V, slots, pos, aim):
        self.tag, self.nh, self.nkv = tag, nh, nkv
        self.q, self.K, self.V = q, K, V
        self.slots, self.pos, self.aim = list(slots), list(pos), aim
        self._ref = None

    @property
    def nq(self):
        return len(self.pos)

    @property
    def ctx(self):
        return self.K.shape[2]

    def ref(self):
        if self._ref is None:       # computed once, shared, never written to
            self._ref = attention_ref(self.q, self.K, self.V, self.slots, self.pos, self.nh, self.nkv)
        return self._ref

    def with_kv(self, K, V):
        return Case(self.tag, self.nh, self.nkv, self.q, K, V, self.slots, self.pos, self.aim)

    def inside(self):
        """[nq, nh]: aimed at a key of the row's own range."""
        return (self.aim >= 0) & (self.aim <= torch.tensor(self.pos)[:, None])

    def past(self):
        return self.aim > torch.tensor(self.pos)[:, None]


def _unit(g, *shape):
    x = torch.randn(*shape, HD, generator=g, dtype=torch.float64)
    return x / x.norm(dim=-1, keepdim=True)


def build_case(tag, nh, nkv, nslot, ctx, rows, seed, extra=()):
    """rows: [(slot, pos, [the key each of the nh heads is aimed at, or -1])]; extra: [(slot, key)] planted
    with no row aimed at them.  A planted key is planted in every kv head of its slot; its direction u
    depends on (kv head, key) alone, so the same key of two slots answers the same query with another V.
    A (row, head) aimed at a key past the row's last is anchored on key 0 as well (q += 10 u_0, a score of
    20): its reference output is key 0's V, exact in bf16 like the other rows', and the key past the end,
    taken in by mistake, still wins by e^10."""
    g = torch.Generator().manual_seed(seed)
    G = nh // nkv
    K = 0.25 * torch.randn(nslot, nkv, ctx, HD, generator=g)
    V = 0.25 * torch.randn(nslot, nkv, ctx, HD, generator=g)
    planted = {(s, e) for s, _, t in rows for e in t if e >= 0} | set(extra)
    planted = sorted(planted | {(s, 0) for s, p, t in rows if max(t) > p})       # the anchor of rows aimed past
    keys = sorted({e for _, e in planted})
    col = {e: j for j, e in enumerate(keys)}
    U = _unit(g, nkv, max(1, len(keys)))
    for s, e in planted:
        assert 0 <= e < ctx, (tag, e, ctx)
        K[s, :, e] = (2.0 * math.sqrt(HD) * U[:, col[e]]).float()
        V[s, :, e] = 24.0 * torch.sign(torch.randn(nkv, HD, generator=g))
    q = torch.randn(len(rows), nh, HD, generator=g)
    aim = torch.full((len(rows), nh), -1, dtype=torch.long)
    for i, (s, p, t) in enumerate(rows):
        assert len(t) == nh and 0 <= p < ctx
        for h, e in enumerate(t):
            if e >= 0:
                q[i, h] = (15.0 * U[h // G, col[e]]).float() + 0.5 * q[i, h]
                if e > p:
                    q[i, h] += (10.0 * U[h // G, col[0]]).float()
                aim[i, h] = e
    return Case(tag, nh, nkv, q.reshape(len(rows), nh * HD).bfloat16(), K.bfloat16(), V.bfloat16(),
                [s for s, _, _ in rows], [p for _, p, _ in rows], aim)


def past_keys(length):
    """Keys past a row of `length` keys that k_attn could take in by mistake: the next one, the eighth,
    the last of the 8-key V group attn_load_v does load, and the first of the next 32-key step."""
    p = length - 1
    return sorted({p + 1, p + 8, p | 7, _r32(p + 1)} - {p})


def planted_rows(nh, nkv, lens_edges, per_head):
    """Rows of one slot aimed at every edge: per (row, kv head) one edge for all its heads, or, per_head,
    one edge per (row, head).  A row's spare places repeat its length's edges."""
    G = nh // nkv
    rows = []
    for length, edges in lens_edges:
        per_row = nh if per_head else nkv
        for r0 in range(0, len(edges), per_row):
            t = [edges[(r0 + j) % len(edges)] for j in range(per_row)]
            rows.append((0, length - 1, t if per_head else [t[h // G] for h in range(nh)]))
    return rows


def planted_case(tag, nh, nkv, lens, chunk, per_head=False, seed=0, nsplit=None):
    """One slot under k_attn's plan `chunk` (0: the default 1,024) for rows of the lengths `lens`: rows
    aimed at every index of split_edges, then rows aimed at the keys past_keys names.  The capacity leaves
    at least a 32-key step past the longest row."""
    c = chunk or 1024
    ns = nsplit or plan_nsplit(max(lens), c)
    le = [(n, split_edges(n, ns, c, plan_waves(c))) for n in lens]
    rows = planted_rows(nh, nkv, le, per_head)
    for n in lens:
        rows += [(0, n - 1, [e] * nh) for e in past_keys(n)]
    ctx = (max(lens) + 8 + 63) // 64 * 64 + 64
    case = build_case(tag, nh, nkv, 1, ctx, rows, seed)
    case.lens_edges, case.nsplit, case.chunk = le, ns, c
    return case


def poisoned(case):
    """The case's K and V with every position past the longest row's last key holding bf16 NaN."""
    K, V = case.K.clone(), case.V.clone()
    K[:, :, max(case.pos) + 1:] = math.nan
    V[:, :, max(case.pos) + 1:] = math.nan
    return K, V


def staircase_keys(nsteps):
    """The planted key of each 32-key step (anywhere in the step; the last two steps' first key)."""
    return [32 * j + ((13 * j + 5) % 32 if j < nsteps - 2 else 0) for j in range(nsteps)]


def staircase_case(step_nats, direction, nh=12, nkv=2, nsteps=8, pos=None, seed=0):
    """Rows whose per-32-key-step maximum rises (direction > 0) or falls by step_nats from step to step:
    one planted key per step, all along one direction u per kv head, with scores step_nats * 1 .. nsteps;
    q = 15 u + noise orthogonal to u, so the planted scores are the graded ones exactly.  pos: the rows'
    positions (default: one row over all 32 * nsteps keys)."""
    g = torch.Generator().manual_seed(seed + 7)
    G = nh // nkv
    ctx = 32 * nsteps
    pos = list(pos) if pos is not None else [ctx - 1]
    K = 0.25 * torch.randn(1, nkv, ctx, HD, generator=g)
    V = 0.25 * torch.randn(1, nkv, ctx, HD, generator=g)
    U = _unit(g, nkv)
    keys = staircase_keys(nsteps)
    score = [step_nats * (j + 1 if direction > 0 else nsteps - j) for j in range(nsteps)]
    for j, e in enumerate(keys):
        K[0, :, e] = (score[j] * math.sqrt(HD) / 15.0 * U).float()
        V[0, :, e] = 24.0 * torch.sign(torch.randn(nkv, HD, generator=g))
    noise = torch.randn(len(pos), nh, HD, generator=g, dtype=torch.float64)
    Uh = U.repeat_interleave(G, 0)                                       # [nh, 128]
    noise -= (noise * Uh).sum(-1, keepdim=True) * Uh
    q = (15.0 * Uh + 0.5 * noise).float()
    aim = torch.full((len(pos), nh), -1, dtype=torch.long)
    for i, p in enumerate(pos):
        seen = [j for j, e in enumerate(keys) if e <= p]
        if seen:
            aim[i, :] = keys[max(seen, key=lambda j: score[j])]
    tag = f"staircase {'+' if direction > 0 else '-'}{step_nats} x {nsteps}"
    case = Case(tag, nh, nkv, q.reshape(len(pos), nh * HD).bfloat16(), K.bfloat16(), V.bfloat16(), [0] * len(pos), pos,
                aim)
    case.keys = keys
    return case


def lazy_max_moves(case, lazy=8.0):
    """k_attn_pf's lazy running max, replayed on the reference's scores: per (row, head) the 32-key steps
    at which the step's max exceeds the running one by more than `lazy` log2 units -> [nq][nh] lists."""
    G = case.nh // case.nkv
    q = case.q.reshape(case.nq, case.nh, HD).double()
    Kd = case.K.double()
    moves = []
    for i, (s, p) in enumerate(zip(case.slots, case.pos)):
        row = []
        for h in range(case.nh):
            sc = (Kd[s, h // G, :p + 1] @ q[i, h]) / math.sqrt(HD) * math.log2(math.e)
            m, mv = -math.inf, []
            for k0 in range(0, p + 1, 32):
                mx = float(sc[k0:k0 + 32].max())
                if mx > m + lazy:
                    m = mx
                    mv.append(k0 // 32)
            row.append(mv)
        moves.append(row)
    return moves


# ------------------------------------------------------------------ the cases of the GPU tests
LAYOUTS = [(12, 2), (28, 4)]
# name -> (chunk (0: default), merge_in values, the lengths sharing the launch, one edge per (row, head))
DECODE_PLANS = {
    "default-1split": (0, (-1,), (1000, 1024), False),      # per = 128: four steps per wave, an 8-key tail
    "default-2splits": (0, (-1,), (1025, 2047), True),      # a 1-key split; the in-kernel merge
    "c32": (32, (-1,), (33, 97, 254, 256), False),          # 32-key splits, fewer active than planned, a 30-key tail
    "c96": (96, (-1,), (161, 190, 191), False),             # per = 64: set B, no reload; 161: a wave with one key
    "c128": (128, (-1, 0), (700, 513), False),              # four waves; waves with no key in the last split
    "c256-merge": (256, (0,), (1500,), False),              # eight waves, per = 32; k_attn_merge with 6 splits
    "c32-merge": (32, (0,), (257, 513, 1280, 8192), True),  # k_attn_merge with 9, 17, 40 and 256 splits
}
# (step in nats, direction, 32-key steps): the issue's three, and a gentle one whose alpha stays visible
STAIRCASES = [(9, 1, 8), (4, 1, 8), (9, -1, 8)]
STAIR_PLANS = [(32, -1), (32, 0), (0, -1)]
# a 1,024-key staircase under the default plan: four carried steps per wave, alpha = e^-2 each
GENTLE = (2, 1, 32)


@functools.lru_cache(maxsize=None)
def decode_case(plan, nh, nkv):
    chunk, _, lens, per_head = DECODE_PLANS[plan]
    return planted_case(f"{plan} {nh}/{nkv}", nh, nkv, lens, chunk, per_head, seed=len(plan) + nh)


@functools.lru_cache(maxsize=None)
def stair_case(step_nats, direction, nsteps, nh=12, nkv=2):
    return staircase_case(step_nats, direction, nh, nkv, nsteps, seed=step_nats + nsteps)


ENGINE_CTX, ENGINE_CHUNK, ENGINE_LENS = 1280, 160, (1280, 1000, 161)


@functools.lru_cache(maxsize=None)
def engine_case():
    """An engine's slot 0 (max_ctx 1,280) under 160-key splits: 8 splits of 4 waves, two steps per wave;
    1,000 keys: 7 active, a 40-key last split; 161: a 1-key split.  Forms 0, 2 and 3 of vv_diag_attn_ctx."""
    case = planted_case("engine 12/2", 12, 2, ENGINE_LENS, ENGINE_CHUNK, True, seed=160,
                        nsplit=plan_nsplit(ENGINE_CTX, ENGINE_CHUNK))
    assert case.ctx >= ENGINE_CTX      # (the longest row fills the engine's context: its past keys do not exist)
    return Case(case.tag, 12, 2, case.q, case.K[:, :, :ENGINE_CTX].contiguous(), case.V[:, :, :ENGINE_CTX].contiguous(),
                case.slots, case.pos, case.aim.masked_fill(case.aim >= ENGINE_CTX, -1)), case.lens_edges


PREFILL_LAYOUTS = [(12, 2), (28, 4), (8, 8)]       # QW = 1, QW = 2, G = 1


def _diag_targets(p):
    b = 32 * (p // 32)
    return [0, p, p - 1, b, b - 1]


@functools.lru_cache(maxsize=None)
def prefill_causal_case(nh, nkv):
    """200 rows of one slot's causal prefill: the row at p is aimed at one of key 0, the diagonal key, the
    one before it and both sides of its last step edge, cycling; every fifth row instead at p + 1, which
    the next row of the same tile has written.  Capacity 256; keys 200 .. 255 are beyond every row: 200
    holds a planted key, finite (the stage's second block, 224 .. 255, is skipped, not masked)."""
    rows = []
    for p in range(200):
        if p % 5 == 4:
            rows.append((0, p, [p + 1] * nh))
        else:
            t = [e for e in _diag_targets(p) if 0 <= e <= p]
            rows.append((0, p, [t[(p // 5 + p) % len(t)]] * nh))
    return build_case(f"prefill causal {nh}/{nkv}", nh, nkv, 1, 256, rows, seed=200 + nh, extra=[(0, 200), (0, 224)])


@functools.lru_cache(maxsize=None)
def prefill_stair_case(step_nats, direction, nh=12, nkv=2):
    return staircase_case(step_nats, direction, nh, nkv, 8, pos=range(192, 256), seed=step_nats)


@functools.lru_cache(maxsize=None)
def prefill_two_slot_case(nh=12, nkv=2):
    """One 32-row tile over two slots: rows 0 .. 19 at positions 100 .. 119 of slot 0, rows 20 .. 31 at
    0 .. 11 of slot 1.  Every key a row is aimed at is planted in the other slot too, with the same
    direction and another V, so a row that read the other slot's key would show it."""
    rows = []
    for i, p in enumerate(range(100, 120)):
        rows.append((0, p, [[i % 12, p, p - 1, 96, 95][i % 5]] * nh))
    for p in range(12):
        rows.append((1, p, [[0, p, max(p - 1, 0)][p % 3]] * nh))
    keys = {e for _, _, t in rows for e in t}
    return build_case("prefill two slots", nh, nkv, 2, 128, rows, seed=31, extra=[(s, e) for s in (0, 1) for e in keys])


@functools.lru_cache(maxsize=None)
def prefill_continuation_case(nh=12, nkv=2):
    """Positions 500 .. 569 over 500 earlier keys: rows aimed into the kfull region (keys every row of the
    tile attends: no mask), at its last step edge, and on the diagonal steps; 570 and 575 are planted past
    nk inside the last computed block, 576 opens the next stage (capacity 640)."""
    rows = []
    for i, p in enumerate(range(500, 570)):
        b = 32 * (p // 32)
        t = [0, 31, 32, 250, 479, 480, 499, 500, b - 1, b, p - 1, p, p + 1]
        rows.append((0, p, [t[i % len(t)]] * nh))
    return build_case("prefill continuation", nh, nkv, 1, 640, rows, seed=570, extra=[(0, 570), (0, 575), (0, 576)])
