"""Case tables, operand builder, fp64 references and the host Philox mask of the exact-arithmetic attention tests
(tests/test_attn_exact.py without a device, tests/test_attn_exact_gpu.py on one).  Imports without a device.

Softmax made exact.  The fused kernels of attn.hip and the softmax kernels of bert.hip compute, per (sequence, head),
    S = alpha Q K^T + bias,  P = softmax(S),  Pd = P * ds,  ctx = Pd V,
    dPd = (dO V^T) * ds,  dot = sum_k P dPd,  dS = P (dPd - dot) alpha,  dQ = dS K,  dK = dS^T Q,  dV = Pd^T dO
with ds the dropout keep scale (0 or 1/(1-p)).  The operands below make every intermediate a dyadic rational of a few bits, so
that every fp32 sum is exact in any order and every 16-bit rounding is the identity; the reference is these formulas in fp64
(never torch.softmax) and the comparison is torch.equal.

Scores.  Head size 64, alpha = 1/8.  A permutation of the 64 dimensions (drawn per case: it moves the groups across the MFMA
k-slots) is split into 32 code dimensions, 15 Q-payload dimensions (K is zero there), 15 K-payload dimensions (Q is zero there),
one shift dimension and one spare (zero).  Every key belongs to a class; its K row holds 32 in the two code dimensions of the
class (a two-hot code: C(32, 2) = 496 classes).  Every query targets one class that has live keys and holds 32 in that class's two
code dimensions.  A raw score is then 256 on a class match, 128 where one code dimension is shared and 0 otherwise: every
non-maximal score is at least 128 below the row maximum, __expf(0) is exactly 1 and __expf(x <= -128) is exactly 0 (2^-184 is
below the smallest fp32 denormal).  Class sizes among the live keys are drawn from {1, 2, 2, 4, 4, 8} (the tail cut to powers of
two): the row sum m is in {1, 2, 4, 8}, 1/m is exact, P is exactly 1/m on the hit set and exactly 0 elsewhere.  Class members are
scattered over the live key positions by a seeded permutation, so hit sets straddle 32-key blocks, 256-key chunks and the keys a
wave owns.

Payloads.  Q and K payload entries are integers in [-3, 3]; V is in {-2 .. 2} and dO in {-1, 0, 1}, each with about 1/8 of the
entries non-zero (a denser draw breaks the 16-bit round trip of dS on some seeds).

Masked keys (padded view) carry the code of a class that also has live members: a kernel that ignored the bias would change m.
Shifted scores (every packed case, some padded ones): the shift dimension holds 32 in every K row and -128 in every Q row, every
real score is then at most -256, and a zero-filled LDS row -- score 0 -- would be the sole row maximum if it were admitted as a
key.  The sequences of a case share the class codes: a key that leaks across cu_seqlens is a hit.  Dropout: p = 0.5 (one case
0.75), keep scale 2 (4).

The keep mask is a host Philox4x32-10 written from the algorithm common_hip.h states: counter (idx8 lo, idx8 hi, stream,
0x5bd1e995), key (seed lo, seed hi), ten rounds, eight 16-bit halves in the order x.lo, x.hi, y.lo, ..., keep iff half >=
(uint32)(p * 65536); element (query, key) of (sequence i, head h) is half key % 8 of idx8 = ((i nh + h) T + query) T/8 + key/8
with the T of the padded layout.  No kernel output enters a reference.

build asserts the exactness conditions on the reference, before any launch: every non-hit score <= max - 128, m a power of
two, Pd / dS / ctx / dQ / dK / dV survive the round trip through bf16 AND f16, every fp32 partial sum of the matmuls fits 24
bits, at least 40 % of the query rows have a non-zero dQ and at least 60 % of the live key rows a non-zero dK.  A seed that
violates one is replaced in the table; a condition is never relaxed."""
import collections
import functools
import itertools

import numpy as np
import torch

from mammo_clip_amd import lib as L

ST = torch.bfloat16 if L.STORAGE == "bf16" else torch.float16        # the 16-bit storage dtype (= ops.BF16)
F64 = torch.float64
HD = 64
ALPHA = 0.125
NEG = -3.4028234663852886e38      # the key bias of a masked key (mc_mask_bias)
SEED, SID = 0x9E3779B97F4A7C15, 7  # dropout seed (both halves non-zero) and stream id of every launch
PAIRS = list(itertools.combinations(range(32), 2))
assert len(PAIRS) == 496


# ------------------------------------------------------------------------------------------------ host Philox
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words -> four such arrays"""
    lo32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & lo32 for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & lo32, p1 >> np.uint64(32), p1 & lo32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def keep8(seed, stream, idx8, p):
    """bool [..., 8]: which of the 8 elements of every group idx8 (an integer array) are kept"""
    idx8 = np.asarray(idx8, dtype=np.uint64)
    words = philox4x32_10(idx8 & np.uint64(0xFFFFFFFF), idx8 >> np.uint64(32), np.uint64(stream), np.uint64(0x5BD1E995),
                          seed & 0xFFFFFFFF, seed >> 32)
    thr = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    halves = []
    for w in words:
        halves += [w & np.uint64(0xFFFF), w >> np.uint64(16)]
    return np.stack(halves, -1) >= thr


def keep_matrix(bh, T, nq, nk, p, seed=SEED, stream=SID):
    """fp64 [nq, nk]: the keep scale (0 or 1/(1-p)) of queries 0..nq-1 x keys 0..nk-1 of probability matrix bh of the padded
    [b, nh, T, T] layout (T % 8 == 0); all ones at p = 0"""
    if p == 0:
        return torch.ones(nq, nk, dtype=F64)
    assert T % 8 == 0
    g = (nk + 7) // 8
    idx8 = (bh * T + np.arange(nq, dtype=np.int64))[:, None] * (T // 8) + np.arange(g, dtype=np.int64)[None, :]
    keep = keep8(seed, stream, idx8, p).reshape(nq, g * 8)[:, :nk]
    return torch.from_numpy(keep).to(F64) * (1.0 / (1.0 - p))


# ------------------------------------------------------------------------------------------------ case tables
# view padded | packed; pairs: the kernel pairs the row runs on (res = mc_attn[_varlen]_*, long = mc_attn[_varlen]_long_*);
# t: the padded T (padded view) or t0 of the [b, t0] token batch (packed view: the dropout index uses t0 rounded up to 8);
# lens: packed sequence lengths; mask none | length | holes; order None | longest | scrambled; extra: alignment rows beyond
# the multiple of 8; sizes: the class sizes drawn; reach: the seam numbers the row is there for (test_attn_exact.py asserts them)
Case = collections.namedtuple("Case", "view pairs seam t b nh lens mask p shift order extra sizes seed reach")
SIZES = (1, 2, 2, 4, 4, 8)
BOTH, LONG = ("res", "long"), ("long",)


def _frozen(reach):
    return tuple(sorted((k, frozenset(v)) for k, v in reach.items()))


def pad(seam, t, b, nh, mask, p, seed, shift=False, pairs=None, sizes=SIZES, **reach):
    return Case("padded", pairs if pairs is not None else (BOTH if t <= 256 else LONG), seam, t, b, nh, None, mask, p, shift, None, 0,
                sizes, seed, _frozen(reach))


def pack(seam, lens, t0, nh, p, seed, order=None, extra=0, pairs=None, **reach):
    return Case("packed", pairs or (BOTH if max(lens) <= 256 else LONG), seam, t0, len(lens), nh, tuple(lens), "none", p, True,
                order, extra, SIZES, seed, _frozen(reach))


# reach: kb = key blocks ceil(len / 32), qb = query blocks ceil(len / 16), chunks = ceil(tp / 256), partial = a last block that
# is not full (packed view); each a set of values that must occur among the row's sequences
PRECONDITION = pad("precondition: classes of 1 and 2, one head", 32, 2, 1, "none", 0.0, 0, sizes=(1, 2), kb={1}, chunks={1})

PADDED = [    # the resident sizes; every row runs on the resident AND the long pair
    pad("T 32: one key block, one wave in phase B", 32, 2, 1, "none", 0.0, 1, kb={1}, qb={2}),
    pad("T 32, length mask, dropout", 32, 3, 3, "length", 0.5, 2, kb={1}),
    pad("T 32, mask with holes", 32, 2, 3, "holes", 0.0, 3, kb={1}),
    pad("T 64: two key blocks", 64, 3, 3, "none", 0.5, 4, kb={2}, qb={4}),
    pad("T 64, length mask", 64, 2, 1, "length", 0.0, 5, kb={2}),
    pad("T 64, holes across key 32, dropout", 64, 2, 3, "holes", 0.5, 6, kb={2}),
    pad("T 160: ten query blocks, second trip partly empty", 160, 2, 3, "none", 0.0, 7, kb={5}, qb={10}),
    pad("T 160, length mask, dropout", 160, 3, 1, "length", 0.5, 8, qb={10}),
    pad("T 160, holes, dropout", 160, 2, 1, "holes", 0.5, 9, qb={10}),
    pad("T 256: two trips, all eight waves own keys", 256, 2, 3, "none", 0.5, 10, kb={8}, qb={16}, chunks={1}),
    pad("T 256, length mask", 256, 3, 1, "length", 0.0, 11, kb={8}),
    pad("T 256, holes", 256, 2, 3, "holes", 0.0, 703, kb={8}),
    pad("T 256, shifted scores, holes, dropout", 256, 2, 1, "holes", 0.5, 13, shift=True, kb={8}),
]

PADDED_LONG = [
    pad("long T 32: tiles shorter than a chunk", 32, 2, 3, "holes", 0.5, 21, kb={1}, chunks={1}),
    pad("long T 256: exactly one chunk", 256, 2, 1, "length", 0.5, 22, kb={8}, chunks={1}),
    pad("long T 288: a second chunk of one block", 288, 2, 3, "none", 0.0, 1259, kb={9}, qb={18}, chunks={2}),
    pad("long T 288, holes on both sides of key 256, dropout", 288, 2, 1, "holes", 0.5, 24, kb={9}, chunks={2}),
    pad("long T 384: a second chunk of four blocks, holes on both sides of key 256, p 0.75", 384, 2, 1, "holes", 0.75, 2007, kb={12}, qb={24}, chunks={2}),
    pad("long T 384, length mask, dropout", 384, 3, 3, "length", 0.5, 1401, chunks={2}),
    pad("long T 512: two full chunks, four query blocks per wave", 512, 3, 3, "none", 0.5, 27, kb={16}, qb={32}, chunks={2}),
    pad("long T 512, holes on both sides of key 256, dropout", 512, 2, 1, "holes", 0.5, 28, kb={16}, chunks={2}),
    pad("long T 512, length mask", 512, 2, 1, "length", 0.0, 1002, kb={16}),
    pad("long T 512, shifted scores, dropout", 512, 2, 1, "none", 0.5, 30, shift=True, kb={16}, chunks={2}),
]

LENS_A = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256)
LENS_B = (33, 1, 256, 64)
LENS_C = (257, 1, 511, 33, 512, 256, 289, 300)
PACKED = [    # max length <= 256: every row runs on the resident AND the long pair
    pack("packed 1..256: lengths around every block edge, alignment rows", LENS_A, 256, 3, 0.0, 2180, extra=8,
         kb={1, 2, 4, 5, 8}, qb={1, 2, 3, 8, 9, 16}, partial={True, False}),
    pack("packed 1..256, t0 257 (T/8 = 33), longest first, dropout", LENS_A, 257, 1, 0.5, 42, order="longest", partial={True}),
    pack("packed 1..256, scrambled order, dropout", LENS_A, 256, 1, 0.5, 43, order="scrambled", extra=16, partial={True}),
    pack("packed [33, 1, 256, 64], t0 257, dropout", LENS_B, 257, 3, 0.5, 44, kb={1, 2, 8}, partial={True, False}),
    pack("packed [33, 1, 256, 64], scrambled order", LENS_B, 257, 1, 0.0, 45, order="scrambled", kb={2}),
    pack("packed [33, 1, 256, 64], longest first", LENS_B, 256, 3, 0.0, 2404, order="longest", extra=8, kb={2}),
]

PACKED_LONG = [
    pack("long packed 1..512 in one call", LENS_C, 512, 1, 0.0, 1000, kb={1, 2, 8, 9, 10, 16}, chunks={1, 2}, partial={True, False}),
    pack("long packed 1..512, longest first, dropout", LENS_C, 512, 3, 0.5, 1001, order="longest", extra=8, chunks={1, 2}),
    pack("long packed [512] alone, dropout", (512,), 512, 3, 0.5, 53, kb={16}, chunks={2}, partial={False}),
    pack("long packed [257] alone: a second chunk of one partial block", (257,), 512, 1, 0.0, 54, kb={9}, chunks={2}, partial={True}),
    pack("long packed [257] alone, t0 300 (T = 304, T/8 = 38), dropout", (257,), 300, 3, 0.5, 55, kb={9}, chunks={2}),
    pack("long packed [300, 257, 33], t0 300, scrambled order, dropout", (300, 257, 33), 300, 1, 0.5, 56, order="scrambled",
         kb={2, 9, 10}, chunks={1, 2}),
]

CASES = [PRECONDITION] + PADDED + PADDED_LONG + PACKED + PACKED_LONG

# the unfused path: (T, p, mask, seed); T 40 / 100 take the general kernels (T/8 no power of two), 64 / 256 / 512 the 8-keys-per-lane
# form with 8 / 32 / 64 lanes per row; dropout needs T % 8 == 0
SOFTMAX = [(40, 0.0, "holes", 61), (40, 0.5, "none", 62), (100, 0.0, "length", 63), (64, 0.0, "none", 64), (64, 0.5, "holes", 65),
           (256, 0.0, "holes", 66), (256, 0.5, "length", 67), (512, 0.0, "none", 5726), (512, 0.5, "holes", 69)]
SOFTMAX_ROWS = 300      # rows of the flattened [b nh T, T] matrices the launches take: no multiple of the rows per wave (1 .. 8)


def softmax_case(T, p, mask, seed):
    b, nh = next(bn for bn in ((2, 1), (2, 3), (3, 3)) if bn[0] * bn[1] * T > SOFTMAX_ROWS)
    return pad(f"unfused T {T} p {p}", T, b, nh, mask, p, seed, pairs=())


def case_id(cs):
    return "".join(ch if ch.isalnum() else "_" for ch in cs.seam).strip("_")


# ------------------------------------------------------------------------------------------------ layout
def t_pad(cs):
    """the T of the padded layout: what the dropout index uses"""
    return cs.t if cs.view == "padded" else -(-cs.t // 8) * 8


def seq_lens(cs):
    return [cs.t] * cs.b if cs.view == "padded" else list(cs.lens)


def row_starts(cs):
    ln = seq_lens(cs)
    return [sum(ln[:i]) for i in range(len(ln))]


def total_rows(cs):
    """rows of the row matrices: b T, or the packed rows with their alignment rows"""
    real = sum(seq_lens(cs))
    return real if cs.view == "padded" else -(-real // 8) * 8 + cs.extra


def order_of(cs):
    """the int32 `order` array of a packed case, or None"""
    if cs.order is None:
        return None
    ln = torch.tensor(cs.lens)
    if cs.order == "longest":
        return torch.sort(ln, descending=True, stable=True).indices.to(torch.int32)
    perm = torch.randperm(len(cs.lens), generator=torch.Generator().manual_seed(cs.seed))
    if perm.tolist() == sorted(perm.tolist()):       # (the draw was the identity)
        perm = perm.roll(1)
    return perm.to(torch.int32)


def live_keys(cs, i):
    """bool [len]: the keys of sequence i that the mask admits"""
    n = seq_lens(cs)[i]
    live = torch.ones(n, dtype=torch.bool)
    if cs.mask == "length":
        live[(n - 7, n // 2 + 3, 9)[i % 3]:] = False
    elif cs.mask == "holes":     # at the start, across every 32- / 256-key boundary the sequence has, and in the last 7 keys
        dead = [0, 1 + i, n - 7, n - 5, n - 4, n - 1]
        for edge in (32, 256):
            if n > edge:
                dead += list(range(edge - 3 - i, edge + 3))
        live[torch.tensor(dead)] = False
    else:
        assert cs.mask == "none"
    return live


def seams(cs):
    """the seam numbers of a row, as sets over its sequences"""
    ln = seq_lens(cs)
    return dict(kb={-(-n // 32) for n in ln}, qb={-(-n // 16) for n in ln}, chunks={-(-(-(-n // 32) * 32) // 256) for n in ln},
                partial={n % 32 != 0 for n in ln})


# ------------------------------------------------------------------------------------------------ operands and reference
def _draw_sizes(n, sizes, g):
    out = []
    while n:
        s = sizes[int(torch.randint(0, len(sizes), (1,), generator=g))]
        if s > n:
            s = 1 << (n.bit_length() - 1)
        out.append(s)
        n -= s
    return out


def _sparse(values, shape, g):
    """entries from `values` with probability 1/8, else 0"""
    v = torch.tensor(values, dtype=F64)[torch.randint(0, len(values), shape, generator=g)]
    return v * (torch.randint(0, 8, shape, generator=g) == 0)


def head_operands(cs, i, h, dims, codes):
    """Q, K, V, dO [len, 64] fp64 of (sequence i, head h) and the key bias [len]"""
    g = torch.Generator().manual_seed((cs.seed * 64 + i) * 8 + h)
    n = seq_lens(cs)[i]
    live = live_keys(cs, i)
    pos = live.nonzero().flatten()
    sizes = _draw_sizes(len(pos), cs.sizes, g)
    assert len(sizes) <= len(codes), "more classes than two-hot codes"
    cls = torch.empty(n, dtype=torch.int64)
    cls[pos[torch.randperm(len(pos), generator=g)]] = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    dead = (~live).nonzero().flatten()
    cls[dead] = torch.randint(0, len(sizes), (len(dead),), generator=g)       # a masked key looks like a live class
    target = torch.randint(0, len(sizes), (n,), generator=g)
    code, qpay, kpay, shift = dims[:32], dims[32:47], dims[47:62], dims[62]
    Q, K = torch.zeros(n, HD, dtype=F64), torch.zeros(n, HD, dtype=F64)
    rows = torch.arange(n)
    for side in (0, 1):
        K[rows, code[codes[cls, side]]] = 32.0
        Q[rows, code[codes[target, side]]] = 32.0
    Q[:, qpay] = torch.randint(-3, 4, (n, 15), generator=g).to(F64)
    K[:, kpay] = torch.randint(-3, 4, (n, 15), generator=g).to(F64)
    if cs.shift:
        K[:, shift], Q[:, shift] = 32.0, -128.0
    V = _sparse((-2.0, -1.0, 1.0, 2.0), (n, HD), g)
    dO = _sparse((-1.0, 1.0), (n, HD), g)
    bias = torch.where(live, 0.0, NEG).to(F64)
    return Q, K, V, dO, bias


def _granule(t):
    """the smallest g with t * 2^g integral"""
    for g in range(40):
        s = t * 2.0 ** g
        if bool((s == s.round()).all()):
            return g
    raise AssertionError("not a dyadic rational of few bits")


def _fits_fp32(a, b, what):
    """every partial sum of a @ b, in any order, is exact in fp32"""
    bits = float((a.abs() @ b.abs()).max()) * 2.0 ** (_granule(a) + _granule(b))
    assert bits < 2 ** 24, f"{what}: partial sums need more than 24 bits"


def survives(t, what):
    for st in (torch.bfloat16, torch.float16):
        assert torch.equal(t.to(st).to(F64), t), f"{what}: not representable in {st}"


Head = collections.namedtuple("Head", "S P Pd dP dS m")
Ref = collections.namedtuple("Ref", "qkv dctx maskb ctx dqkv lse heads dq_rows dk_rows")


def head_reference(Q, K, V, dO, bias, ds, what):
    """the kernels' formulas in fp64 -> (ctx, dQ, dK, dV, row max, 1/m, Head); asserts the exactness conditions"""
    S = ALPHA * (Q @ K.T) + bias[None, :]
    mx = S.max(1).values
    hit = S == mx[:, None]
    assert bool((S[~hit] <= (mx[:, None] - 128.0).expand_as(S)[~hit]).all()), f"{what}: a non-maximal score within 128 of the maximum"
    m = hit.sum(1)
    assert bool(((m & (m - 1)) == 0).all()) and int(m.max()) <= 8, f"{what}: a row sum that is no power of two"
    P = hit.to(F64) / m[:, None].to(F64)
    Pd = P * ds
    ctx = Pd @ V
    dP = dO @ V.T
    dPd = dP * ds
    dot = (P * dPd).sum(1)
    dS = P * (dPd - dot[:, None]) * ALPHA
    dQ, dK, dV = dS @ K, dS.T @ Q, Pd.T @ dO
    for name, t in (("Pd", Pd), ("dS", dS), ("ctx", ctx), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        survives(t, f"{what} {name}")
    _fits_fp32(Q, K.T, f"{what} Q K^T")
    _fits_fp32(dO, V.T, f"{what} dO V^T")
    _fits_fp32(P, dPd.T, f"{what} row dots")
    _fits_fp32(Pd, V, f"{what} ctx")
    _fits_fp32(dS, K, f"{what} dQ")
    _fits_fp32(dS.T, Q, f"{what} dK")
    _fits_fp32(Pd.T, dO, f"{what} dV")
    return ctx, dQ, dK, dV, mx, 1.0 / m.to(F64), Head(S, P, Pd, dP, dS, m)


def build(cs, keep_heads=False, coverage=True):
    """Operands and reference of a case in the layout of its view, fp64 on the CPU:
    qkv [R, 3H], dctx [R, H], maskb [b, T] (padded) or None, ctx [R, H], dqkv [R, 3H], lse [b nh T, 2] (padded) or [R, nh, 2]
    (packed; alignment rows NaN); alignment rows of qkv / dctx are NaN, of ctx / dqkv zero.  heads: the per-head matrices
    (keep_heads) in the order of the padded [b, nh, T, T] layout.  Asserts the conditions (module docstring); coverage=False
    leaves out the two on non-zero gradient rows, for the precondition row, whose launches are forward only."""
    gc = torch.Generator().manual_seed(cs.seed)
    dims = torch.randperm(HD, generator=gc)
    codes = torch.tensor(PAIRS)[torch.randperm(len(PAIRS), generator=gc)]
    nh, H, T = cs.nh, cs.nh * HD, t_pad(cs)
    R, lens, r0s = total_rows(cs), seq_lens(cs), row_starts(cs)
    real = sum(lens)
    qkv, dctx = torch.full((R, 3 * H), float("nan"), dtype=F64), torch.full((R, H), float("nan"), dtype=F64)
    ctx, dqkv = torch.zeros(R, H, dtype=F64), torch.zeros(R, 3 * H, dtype=F64)
    padded = cs.view == "padded"
    lse = torch.full((cs.b * nh * T, 2) if padded else (R, nh, 2), float("nan"), dtype=F64)
    maskb = torch.zeros(cs.b, T, dtype=F64) if padded else None
    heads, dq_rows, dk_rows, live_rows = [], 0, 0, 0
    for i, (n, r0) in enumerate(zip(lens, r0s)):
        for h in range(nh):
            what = f"{cs.seam}: sequence {i} head {h}"
            Q, K, V, dO, bias = head_operands(cs, i, h, dims, codes)
            ds = keep_matrix(i * nh + h, T, n, n, cs.p)
            c, dQ, dK, dV, mx, inv, hd = head_reference(Q, K, V, dO, bias, ds, what)
            live = bias == 0
            assert not bool(dK[~live].any()) and not bool(dV[~live].any()), f"{what}: a masked key with a gradient"
            cols = slice(h * HD, (h + 1) * HD)
            for part, (x, dx) in enumerate(((Q, dQ), (K, dK), (V, dV))):
                qkv[r0:r0 + n, part * H + h * HD:part * H + (h + 1) * HD] = x
                dqkv[r0:r0 + n, part * H + h * HD:part * H + (h + 1) * HD] = dx
            dctx[r0:r0 + n, cols], ctx[r0:r0 + n, cols] = dO, c
            if padded:
                lse[(i * nh + h) * T:(i * nh + h + 1) * T] = torch.stack([mx, inv], 1)
                maskb[i] = bias
            else:
                lse[r0:r0 + n, h] = torch.stack([mx, inv], 1)
            dq_rows += int(dQ.any(1).sum())
            dk_rows += int(dK.any(1).sum())
            live_rows += int(live.sum())
            if keep_heads:
                heads.append(hd)
    assert not coverage or dq_rows >= 0.4 * real * nh, f"{cs.seam}: only {dq_rows} of {real * nh} query rows have a non-zero dQ"
    assert not coverage or dk_rows >= 0.6 * live_rows, f"{cs.seam}: only {dk_rows} of {live_rows} live key rows have a non-zero dK"
    return Ref(qkv, dctx, maskb, ctx, dqkv, lse, heads, dq_rows / (real * nh), dk_rows / live_rows)


@functools.lru_cache(maxsize=2)
def reference(cs):
    """build(cs), shared by the tests of a row; treat it as read-only"""
    return build(cs, coverage=cs is not PRECONDITION)
