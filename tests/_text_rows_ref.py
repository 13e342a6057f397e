"""Shared by tests/test_text_rows_ref.py (CPU) and tests/test_text_rows_fp64_gpu.py: fp64 references of the text-tower row kernels
of csrc/bert.hip (embedding + LayerNorm, dropout + add + LayerNorm, masked softmax with dropout, erf-GELU; forward and backward),
an a-priori error bound PER ELEMENT for each of their outputs, and wrong variants ("controls") that the bounds must reject.  No
kernel output enters anything here; everything is torch fp64 on whatever device the inputs live on, computed from the same
16-bit-rounded activations (ops.BF16: bf16, f16 under MC_STORAGE=f16) and the same fp32 parameters the kernel reads.  Dropout
masks come from the host Philox of tests/_attn_exact_cases.py through keep_mask / keep_scale of tests/_mlp_head_common.py.

Bounds.  U = 2^-24 is the unit round-off of one fp32 operation; "terms" are the addends of an expression, so that the bound of a
cancelling expression is relative to what was added and not to what is left.  hu(v) = half a 16-bit ulp of the binade of the
reference value v (7 mantissa bits for bf16, 10 for f16; not under the smallest normal binade); every 16-bit output carries it.
TINY = 2^-126 is added wherever an fp32 intermediate may be flushed as a denormal.  L = 8 * ceil(h / 512) + 6 is the longest fp32
chain of a LayerNorm row sum (8 elements of a vector, 1 or 2 vectors per lane, six wave-reduction steps), LS = 8 + 6 that of a
softmax row sum (at most 8 keys per lane).
  s       the LayerNorm input k x + res (k = keep scale) or word + type + pos.  e_s = U * (|k x| + |s|) resp. 2 U * (|word| + |type| +
          |pos|): one rounding per operation; 0 where the reference finds k x + res exactly representable in fp32 at p = 0 (an
          exact sum is not rounded).  A = the sum of the |terms| of s.
  mean    (L + 8) U * mean(A), absolute: L roundings of the sum, the division, the roundings of s itself.
  rstd    relative: (L + 8) U + [sum |d| e_s + 0.5 sum (e_s + e_mean + U |d|)^2] / (sum d^2 + h eps), d = s - mean.  The first
          term is half of the (L + 4) U of the sum of squares and the division, plus rsqrt (1 ulp), eps + var and the cast of eps;
          an error of the mean enters the variance in second order only (sum d = 0), which the squared term carries with the
          second order of e_s.  The middle term is the first-order effect of the rounded s: it is 0 for exact s, ~U for unit
          normal rows, and is what makes rows of mean 64 and sd 0.5 hard when their s is NOT exact.
  xhat    e_xh = rstd (e_s + e_mean + U |d|) + |xhat| (e_rstd + 2 U): the shift by the mean error, the statistics, two roundings.
  y       hu(y) + |gamma| e_xh + 4 U (|xhat gamma| + |beta|); the embedding multiplies by k afterwards: k times that + U |y|.
  dres    the LayerNorm input gradient rstd (g - s1 - xhat s2), g = dy gamma, s1 = mean(g), s2 = mean(g xhat):
          e_s1 = (L + 8) U mean|g|, e_s2 = (L + 8) U mean|g xhat| + mean(|g| e_xh),
          e_in = U |g| + e_s1 + |xhat| e_s2 + e_xh |s2| + e_xh e_s2 + 3 U (|g| + |s1| + |xhat s2|),
          e_dres = rstd e_in (1 + e_rstd) + |dres| (e_rstd + U), and hu(dres) where it is stored in 16 bits.
  dx      k dres: k e_dres + U |dx| + hu(dx).
  sums    dgamma, dbeta, dword[id], dpos[t], dtype[ty], PER ENTRY: (n + 64) U S + E.  S = fp64 sum of |term| over the n rows that
          contribute a non-zero term; n U S is the worst case of an fp32 sum of n terms in ANY order, so it covers the atomic
          endings, the per-wave partial sums and the fp64 ordered sums of the store-and-sum endings alike; 64 U S covers the
          roundings inside a term; E = the sum over the rows of the error of the term that the row inherits from xhat / dres
          (|dy| e_xh for dgamma, e_dres for the embedding tables, 0 for dbeta).
  softmax p = e / sum e, e = __expf(a), a = s - max <= 0: relative e_e = U (|a| + 2 |a| log2(e) + 2): the subtraction, the
          argument scaling a * log2(e) of the fast exponential (an absolute error of the exponent is a relative error of the
          result), v_exp_f32 and one product.  e_p = p (e_e + sum_j p_j e_e_j + (LS + 4) U) + hu(p) + TINY.
  dscores p (k dp - dot) alpha, dot = sum p k dp: alpha |p| ((LS + 4) U sum |p k dp| + 4 U (|k dp| + |dot|)) + hu + TINY.
  GELU    hu + 8 U |x|: erff is good to a few ulp of ITS result, so 1 + erf carries an absolute error of a few U which the
          product with 0.5 x scales by |x| -- not by the (possibly tiny) result.
  GELU'   hu + (8 U (|cdf| + |x pdf|) + 4 U |erf(x / sqrt 2)|) |dy|.  The second term is that same absolute error of 1 + erf
          in cdf = 0.5 (1 + erf): a bound relative to |cdf| + |x pdf| alone cannot hold in the far negative tail, where both
          vanish and the error of erff (relative to |erf| = 1) does not.

Controls, from the reference alone (test_text_rows_ref.py asserts the shares): single-pass fp32 variance on rows of mean 64 and
sd 0.5; a softmax whose row sum leaves out the last key; the tanh approximation of GELU; a column sum with one row dropped."""
import math

import numpy as np
import torch

from _attn_exact_cases import ST, NEG, keep8  # noqa: F401  (keep8: the one host Philox)
from _mlp_head_common import keep_mask, keep_scale

F64 = torch.float64
F32 = torch.float32
U = 2.0 ** -24
TINY = 2.0 ** -126
MANT, EMIN = (7, -126) if ST == torch.bfloat16 else (10, -14)
LOG2E = math.log2(math.e)
SQRT2 = math.sqrt(2.0)
LS = 8 + 6
SEED, SID = 0x9E3779B97F4A7C15, 7          # both 32-bit halves of the seed non-zero, a non-zero stream id


def half_ulp16(ref):
    """half a unit in the last place of the 16-bit storage type in the binade of each (fp64) reference value"""
    _, e = torch.frexp(ref.abs())                                    # |ref| = m 2^e, 0.5 <= m < 1
    e = torch.clamp(e.to(F64) - 1.0, min=float(EMIN))
    return torch.exp2(e - MANT - 1)


def lchain(h):
    return 8 * (-(-h // 512)) + 6


def eps32(eps):
    return float(np.float32(eps))


def rows_keep_scale(drow, h, p, seed=SEED, sid=SID, device="cpu"):
    """fp64 [len(drow), h] keep scale of the rows whose dropout row index (the row of the padded layout) is drow (a host int64
    tensor); rows with drow < 0 are not dropped"""
    drow = torch.as_tensor(drow, dtype=torch.int64).cpu()
    if p == 0:
        return torch.ones(len(drow), h, dtype=F64, device=device)
    full = keep_scale(int(drow.max()) + 1, h, p, seed, sid)
    out = full[drow.clamp(min=0)]
    out[drow < 0] = 1.0
    return out.to(device)


# ------------------------------------------------------------------------------------------------ LayerNorm
class LN:
    """reference and bounds of one LayerNorm forward over the rows of s"""


def _ln(s, A, e_s, gamma, beta, eps):
    h = s.shape[1]
    L = lchain(h)
    o = LN()
    o.h, o.L, o.s, o.e_s = h, L, s, e_s
    o.gamma, o.beta = gamma, beta
    o.mean = s.mean(1)
    o.e_mean = (L + 8) * U * A.mean(1)
    d = s - o.mean[:, None]
    ss = (d * d).sum(1)
    var = ss / h
    o.rstd = 1.0 / torch.sqrt(var + eps)
    o.var = var
    second = (e_s + o.e_mean[:, None] + U * d.abs()) ** 2
    o.e_rstd_rel = (L + 8) * U + ((d.abs() * e_s).sum(1) + 0.5 * second.sum(1)) / (ss + h * eps)
    o.e_rstd = o.e_rstd_rel * o.rstd
    r = o.rstd[:, None]
    o.d = d
    o.xhat = d * r
    o.e_xhat = r * (e_s + o.e_mean[:, None] + U * d.abs()) + o.xhat.abs() * (o.e_rstd_rel[:, None] + 2 * U)
    o.y = o.xhat * gamma + beta
    o.e_y32 = gamma.abs() * o.e_xhat + 4 * U * ((o.xhat * gamma).abs() + beta.abs())
    o.e_y = o.e_y32 + half_ulp16(o.y)
    return o


def add_ln_fwd(x, res, gamma, beta, eps, keep=None):
    """y = LN(keep x + res): x / res 16-bit, gamma / beta fp32, keep the fp64 keep scale or None (p = 0)"""
    x, res, gamma, beta = x.to(F64), res.to(F64), gamma.to(F64), beta.to(F64)
    kx = x if keep is None else x * keep
    s = kx + res
    if keep is None:
        e_s = U * s.abs() * (s.to(F32).to(F64) != s)
    else:
        e_s = U * (kx.abs() + s.abs())
    o = _ln(s, kx.abs() + res.abs(), e_s, gamma, beta, eps32(eps))
    o.keep = keep
    return o


def embed_fwd(ids, pos_ids, tt, word, pos, typ, gamma, beta, eps, keep=None):
    """y = keep LN(word[id] + type[tt] + pos[t]) over flattened token rows; tables fp32; tt None: type 0"""
    word, pos, typ, gamma, beta = (t.to(F64) for t in (word, pos, typ, gamma, beta))
    ty = torch.zeros_like(ids) if tt is None else tt
    a, b, c = word[ids], pos[pos_ids], typ[ty]
    A = a.abs() + b.abs() + c.abs()
    o = _ln(a + c + b, A, 2 * U * A, gamma, beta, eps32(eps))
    o.keep, o.ids, o.pos_ids, o.ty = keep, ids, pos_ids, ty
    o.n_vocab, o.n_pos = word.shape[0], pos.shape[0]
    o.y_ln, o.e_y_ln32 = o.y, o.e_y32
    if keep is not None:
        o.y = o.y_ln * keep
        o.e_y32 = keep * o.e_y_ln32 + U * o.y.abs()
    o.e_y = o.e_y32 + half_ulp16(o.y)
    return o


def col_sum(terms, e_terms=None, index=None, n_index=None):
    """(value, S, n, E) of the sum of `terms` [rows, h] over the rows, per column -- or per (index[row], column) with n_index
    index values: S = sum |term|, n = number of non-zero terms, E = sum of the inherited errors e_terms"""
    def red(t):
        if index is None:
            return t.sum(0)
        return torch.zeros(n_index, t.shape[1], dtype=F64, device=t.device).index_add_(0, index, t)
    return (red(terms), red(terms.abs()), red((terms != 0).to(F64)),
            red(e_terms) if e_terms is not None else torch.zeros_like(red(terms)))


def sum_bound(entry):
    _, S, n, E = entry
    return (n + 64) * U * S + E


def ln_bwd(o, dy):
    """closed-form LayerNorm backward on the forward `o` with the upstream gradient dy (16-bit): dict of per-element
    (value, bound) for dres / dx and of col_sum entries for the sums.  add_ln: dres = dLN, dx = keep dLN.  embedding: dy is
    multiplied by keep first, the tables collect dLN."""
    dy = dy.to(F64)
    emb = hasattr(o, "ids")
    k = o.keep
    d = dy if (not emb or k is None) else dy * k
    h, L = o.h, o.L
    r, xh, exh = o.rstd[:, None], o.xhat, o.e_xhat
    g = d * o.gamma
    s1 = g.mean(1, keepdim=True)
    s2 = (g * xh).mean(1, keepdim=True)
    e_s1 = (L + 8) * U * g.abs().mean(1, keepdim=True)
    e_s2 = (L + 8) * U * (g * xh).abs().mean(1, keepdim=True) + (g.abs() * exh).mean(1, keepdim=True)
    inner = g - s1 - xh * s2
    e_in = U * g.abs() + e_s1 + xh.abs() * e_s2 + exh * s2.abs() + exh * e_s2 + 3 * U * (g.abs() + s1.abs() + (xh * s2).abs())
    dln = r * inner
    er = o.e_rstd_rel[:, None]
    e_dln = r * e_in * (1 + er) + dln.abs() * (er + U)
    out = {"dgamma": col_sum(d * xh, d.abs() * exh), "dbeta": col_sum(d)}
    if emb:
        nv, npos = o.n_vocab, o.n_pos
        out["dword"] = col_sum(dln, e_dln, o.ids, nv)
        out["dpos"] = col_sum(dln, e_dln, o.pos_ids, npos)
        out["dtype"] = col_sum(dln, e_dln, o.ty, 2)
        out["dln"] = (dln, e_dln)
        return out
    out["dres"] = (dln, e_dln + half_ulp16(dln))
    dx = dln if k is None else dln * k
    e_dx = e_dln if k is None else k * e_dln + U * dx.abs()
    out["dx"] = (dx, e_dx + half_ulp16(dx))
    return out


# ------------------------------------------------------------------------------------------------ softmax
def softmax_fwd(scores):
    """(p, bound) of the row softmax of fp32 scores [rows, t]"""
    s = scores.to(F64)
    a = s - s.max(1, keepdim=True).values
    e = torch.exp(a)
    p = e / e.sum(1, keepdim=True)
    ee = U * (a.abs() + 2 * a.abs() * LOG2E + 2)
    ee = torch.where(p > 0, ee, torch.zeros_like(ee))              # (a key at -FLT_MAX under a finite maximum: exactly 0)
    bound = p * (ee + (p * ee).sum(1, keepdim=True) + (LS + 4) * U) + half_ulp16(p) + TINY
    return p, bound


def softmax_bwd(probs16, dpd, alpha, keep=None):
    """(dscores, bound) from the 16-bit probabilities the kernel reads, the fp32 gradient of the dropped probabilities and the
    keep scale"""
    p, d = probs16.to(F64), dpd.to(F64)
    if keep is not None:
        d = d * keep
    dot = (p * d).sum(1, keepdim=True)
    ds = p * (d - dot) * alpha
    bound = abs(alpha) * p * ((LS + 4) * U * (p * d).abs().sum(1, keepdim=True) + 4 * U * (d.abs() + dot.abs())) + half_ulp16(ds) + TINY
    return ds, bound


# ------------------------------------------------------------------------------------------------ GELU
def gelu_fwd(x):
    x = x.to(F64)
    y = 0.5 * x * torch.special.erfc(-x / SQRT2)                    # 1 + erf(t) = erfc(-t): no cancellation in the reference
    return y, half_ulp16(y) + 8 * U * x.abs()


def gelu_grad(x):
    """(cdf + x pdf, cdf, x pdf) in fp64"""
    x = x.to(F64)
    cdf = 0.5 * torch.special.erfc(-x / SQRT2)
    xpdf = x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    xpdf = torch.where(torch.isfinite(xpdf), xpdf, torch.zeros_like(xpdf))
    return cdf + xpdf, cdf, xpdf


def gelu_bwd(x, dy):
    dy = dy.to(F64)
    g, cdf, xpdf = gelu_grad(x)
    dx = dy * g
    bound = half_ulp16(dx) + (8 * U * (cdf.abs() + xpdf.abs()) + 4 * U * torch.erf(x.to(F64) / SQRT2).abs()) * dy.abs()
    return dx, bound


def all_finite_patterns(device="cpu"):
    """every finite value of the 16-bit storage type that is zero or normal (both signs), padded with zeros to a multiple of 8"""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    mant_bits, exp_mask = (7, 0xFF) if ST == torch.bfloat16 else (10, 0x1F)
    ex = (bits >> mant_bits) & exp_mask
    ok = ((ex != 0) & (ex != exp_mask)) | ((bits & 0x7FFF) == 0)
    v = bits[ok].to(torch.int16).view(ST)
    pad = (-v.numel()) % 8
    return torch.cat([v, torch.zeros(pad, dtype=ST)]).to(device)


# ------------------------------------------------------------------------------------------------ comparison
def ratio(got, ref, bound):
    """worst |got - ref| / bound over the elements (0 / 0 counts as 0; any error over a zero bound as inf)"""
    err = (got.to(F64) - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(q.max()) if q.numel() else 0.0


def violations(got, ref, bound):
    """share of the elements whose error exceeds the bound"""
    return float(((got.to(F64) - ref).abs() > bound).to(F64).mean())


# ------------------------------------------------------------------------------------------------ inputs
def randn(*shape, seed, scale=1.0, shift=0.0, dtype=None, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g, dtype=F64) * scale + shift
    return t.to(ST if dtype is None else dtype).to(device)


def ln_inputs(kind, rows, h, seed, device="cpu"):
    """(x, res) of the 16-bit storage type for the LayerNorm cases: "normal" unit normal; "offset" rows of mean 64 and sd 0.5 (x
    carries 64 and the 16-bit grid of that binade, res the sd: the sum is exact in fp32); "const" constant rows of small
    integers (variance exactly 0); "spike" one non-zero element per row"""
    if kind == "normal":
        return randn(rows, h, seed=seed, device=device), randn(rows, h, seed=seed + 1, device=device)
    if kind == "offset":
        return (randn(rows, h, seed=seed, scale=0.35, shift=64.0, device=device),
                randn(rows, h, seed=seed + 1, scale=0.35, device=device))
    if kind == "const":
        v = (torch.arange(rows, dtype=F64) % 7 - 3)[:, None].expand(rows, h)
        return (v + 2).to(ST).to(device).contiguous(), torch.full((rows, h), -2.0, dtype=ST, device=device)
    if kind == "spike":
        x = torch.zeros(rows, h, dtype=F64)
        x[torch.arange(rows), (torch.arange(rows) * 131 + 5) % h] = (torch.arange(rows, dtype=F64) % 5 + 1) * 1.5
        return x.to(ST).to(device), torch.zeros(rows, h, dtype=ST, device=device)
    raise ValueError(kind)


def affine(h, seed, device="cpu"):
    """fp32 (gamma around 1, beta around 0)"""
    return (randn(h, seed=seed, scale=0.2, shift=1.0, dtype=F32, device=device),
            randn(h, seed=seed + 1, scale=0.2, dtype=F32, device=device))


def embed_case(b, t, h, with_tt, seed, vocab=50, lengths=None):
    """token batch of the embedding tests (host tensors): every sequence starts with id 1 and ends in a run of id 0, ids 7 and
    vocab - 1 are never named; lengths (packed view): the real tokens of each sequence, else all t.
    -> dict ids [b, t], tt [b, t] | None, lengths, word / pos / typ fp32 tables"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, vocab - 1, (b, t), generator=g)
    ids[ids == 7] = 8
    lengths = [t] * b if lengths is None else list(lengths)
    for i, n in enumerate(lengths):
        ids[i, max(1, n - max(1, n // 4)):] = 0                      # the trailing run of id 0 of the real tokens (and the padding)
        ids[i, 0] = 1
    tt = None
    if with_tt:
        tt = torch.zeros(b, t, dtype=torch.int64)
        for i, n in enumerate(lengths):
            tt[i, n // 2:] = i % 2                                    # odd sequences switch to type 1 half-way
    return {"ids": ids, "tt": tt, "lengths": lengths, "unused": (7, vocab - 1),
            "word": randn(vocab, h, seed=seed + 1, dtype=F32), "pos": randn(max(t, 2), h, seed=seed + 2, scale=0.5, dtype=F32),
            "typ": randn(2, h, seed=seed + 3, scale=0.5, dtype=F32)}


def softmax_scores(rows, t, seed, sd=1.0, offset=0.0, device="cpu"):
    """fp32 scores; from row 1 on the tail of the row past (t * 3) // 4 is masked with the value mc_mask_bias writes, the LAST row
    (rows >= 3) has every key masked and the one before it a single live key (key t // 2)"""
    s = randn(rows, t, seed=seed, scale=sd, shift=offset, dtype=F32)
    if t > 1:
        s[1:, max(1, (t * 3) // 4):] = NEG
    if rows >= 3:
        s[-2] = NEG
        s[-2, t // 2] = float(randn(1, seed=seed + 9, scale=sd, shift=offset, dtype=F32))
        s[-1] = NEG
    return s.to(device)
