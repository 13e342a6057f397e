"""Shared by tests/test_mlp_head.py (CPU) and tests/test_mlp_head_gpu.py: the fp64 restatement of the MLP projection head
[ref: model/modules/projection.py:4-20] and the host Philox mask of its dropout.  No kernel output enters anything here."""
import math
import os

import numpy as np
import torch

from _attn_exact_cases import keep8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_head.npz")
F64 = torch.float64
EPS = 1e-5
PARAMS = ("projection.weight", "projection.bias", "fc.weight", "fc.bias", "layer_norm.weight", "layer_norm.bias")
LOSS_CFG = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}


def cfg(head, dropout=0.1):
    """the B2 + BERT-base model config of the model-level tests with projection head ``head`` ("linear" | "mlp")"""
    return {"name": "clip_custom", "temperature": 0.07,
            "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
            "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                             "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
            "projection_head": {"name": head, "dropout": dropout, "proj_dim": 512}}


def mlp_state_dict(seed=10):
    """a synthetic reference-layout state dict of B2 + BERT-base + MLP heads: the linear-head layout of oracle/weights.py with
    the two heads' fc / layer_norm entries added (seeded, gamma around 1)"""
    from oracle import arch as oarch, bert as obert, weights as ow
    sd = ow.synth_state_dict(ow.clip_shapes(oarch.build_arch("efficientnet-b2"), obert.BertShape()), seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for head in ("image_projection", "text_projection"):
        sd[f"{head}.fc.weight"] = torch.randn(512, 512, generator=g) * 512 ** -0.5
        sd[f"{head}.fc.bias"] = torch.randn(512, generator=g) * 0.1
        sd[f"{head}.layer_norm.weight"] = 1.0 + 0.2 * torch.randn(512, generator=g)
        sd[f"{head}.layer_norm.bias"] = 0.1 * torch.randn(512, generator=g)
    return sd


def keep_mask(rows, n, p, seed, stream):
    """bool [rows, n]: element (row, col) is kept -- half col % 8 of Philox draw (row * n + col) / 8, n % 8 == 0; all True at p = 0"""
    if p == 0:
        return np.ones((rows, n), dtype=bool)
    assert n % 8 == 0
    idx8 = np.arange(rows * n // 8, dtype=np.int64)
    return keep8(int(seed), int(stream), idx8, p).reshape(rows, n)


def keep_scale(rows, n, p, seed, stream, device="cpu"):
    """fp64 [rows, n]: 0 or 1 / (1 - p) with both p and the quotient rounded as the kernel rounds them (fp32)"""
    inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return (torch.from_numpy(keep_mask(rows, n, p, seed, stream)).to(F64) * inv).to(device)


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ln_fwd64(f, res, gamma, beta, scale, eps=EPS):
    """the last two formula lines in fp64 -> (y, xhat, rstd, z)"""
    z = f * scale + res
    mean = z.mean(1, keepdim=True)
    var = ((z - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * rstd
    return xhat * gamma + beta, xhat, rstd.reshape(-1), z


def head64(x, w, scale, eps=EPS):
    """the five formula lines in fp64; w: dict of the six parameters (fp64); scale: keep scale [m, n] or 1.0"""
    p = x @ w["projection.weight"].T + w["projection.bias"]
    g = gelu64(p)
    f = g @ w["fc.weight"].T + w["fc.bias"]
    return ln_fwd64(f, p, w["layer_norm.weight"], w["layer_norm.bias"], scale, eps)[0]


def head64_grads(x, w, cot, scale, eps=EPS):
    """(out, {"x": dx, parameter name: gradient}) of sum(out * cot) by fp64 autograd over head64"""
    x = x.detach().clone().requires_grad_(True)
    w = {k: v.detach().clone().requires_grad_(True) for k, v in w.items()}
    out = head64(x, w, scale, eps)
    (out * cot).sum().backward()
    grads = {"x": x.grad}
    grads.update({k: v.grad for k, v in w.items()})
    return out.detach(), grads


def load_golden():
    z = np.load(GOLDEN)
    w = {k: torch.from_numpy(z["w/" + k]) for k in PARAMS}
    g = {k: torch.from_numpy(z["grad/" + k]) for k in PARAMS + ("x",)}
    return torch.from_numpy(z["x"]), w, torch.from_numpy(z["cotangent"]), torch.from_numpy(z["out"]), g


# ------------------------------------------------------------------------------------------------ forward-error algebra
# A-priori bounds of the fp32 kernels against the fp64 restatement, per element, in the manner of
# tests/test_bnact_family_gpu.py: (chain length + a few) * 2^-24 * sum |terms|, with the error of every intermediate carried
# into what consumes it (a value enters a later sum with its own bound, not with its possibly cancelled size).  Everything is
# computed from the fp64 reference and the shapes alone.  U = 2^-24 is the unit round-off of one fp32 operation.
U = 2.0 ** -24
# erff and the fast __expf of the device library, worst error in units of the last place of the fp32 result, measured on an
# MI355X with scripts/device_math_ulp.hip over |t| <= 4.5 resp. -20.25 <= a <= 0 (ROCm's installed documentation gives no figure):
# erff 1.466 ulp (at t = -0.00173), __expf 15.827 ulp (at a = -20.107: the fast form rounds a * log2(e) before v_exp_f32, an
# error that grows with |a|).  The bounds allow twice that.
ERF_ULP = 2 * 1.466
EXP_ULP = 2 * 15.827
SQRT2 = math.sqrt(2.0)


def lane_chain(n):
    """longest fp32 accumulation chain of a row sum in the row kernels: 8 elements per vector, 1 / 2 / 4 vectors per lane, six
    wave-reduction steps, the division by n"""
    return 8 * (1 if n <= 512 else 2 if n <= 1024 else 4) + 6 + 1


def _erf_err(x):
    t = x / SQRT2
    return ERF_ULP * 2 * U * torch.erf(t).abs() + 2.0 / math.sqrt(math.pi) * torch.exp(-t * t) * 2 * U * t.abs()


def gelu_err(x):
    """bound of the kernel's 0.5 x (1 + erff(x c)) on an exact fp32 x: erff's own error, the rounded argument x c (two
    roundings, through erf' = 2 / sqrt(pi) exp(-t^2)), the rounding of 1 + erf and of the product"""
    s = 1.0 + torch.erf(x / SQRT2)
    return (0.5 * x).abs() * (_erf_err(x) + U * s.abs()) + 2 * U * (0.5 * x * s).abs()


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / SQRT2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_grad_err(x):
    """bound of cdf + x pdf: cdf as in gelu_err; pdf = c * __expf(a), a = -x^2 / 2 rounded once (relative error U |a| of the
    result), __expf's own error, the constant and its product; then the product with x and the sum"""
    s = 1.0 + torch.erf(x / SQRT2)
    a = 0.5 * x * x
    pdf = torch.exp(-a) / math.sqrt(2.0 * math.pi)
    e_cdf = 0.5 * (_erf_err(x) + U * s.abs())
    e_pdf = pdf * (U * a + EXP_ULP * 2 * U + 2 * U)
    return e_cdf + x.abs() * e_pdf + 2 * U * (0.5 * s.abs() + (x * pdf).abs())


def sgemm_chain(m, n, k):
    """longest fp32 accumulation chain of mc_sgemm on an [m, k] x [k, n] product: k sequential fmas in one thread, or, where
    the launcher splits K (read from its own workspace size), the longest split's share plus the in-order sum of the splits"""
    import mammo_clip_amd.lib as L
    splits = max(1, int(L.load().mc_sgemm_ws_floats(m, n, k)) // (m * n))
    return k if splits == 1 else (-(-k // splits) + 31) // 32 * 32 + splits


def gemm_err(a, ea, b, eb, bias=None, chain=None):
    """bound of an fp32 dot-product kernel on C = a @ b (+ bias): ``chain`` (default k: sequential fmas of one thread)
    accumulation steps per output, the epilogue's few roundings"""
    k = a.shape[1] if chain is None else chain
    mag = a.abs() @ b.abs()
    if bias is not None:
        mag = mag + bias.abs()
    return ea @ b.abs() + a.abs() @ eb + ea @ eb + (k + 4) * U * mag


def ln_fwd(f, ef, res, eres, gamma, beta, scale, eps=EPS):
    """reference and bounds of mc_mlp_head_ln_fwd: dict name -> (fp64 value, bound) for y, xhat, rstd"""
    n = f.shape[1]
    Lr = lane_chain(n)
    y, xhat, rstd, z = ln_fwd64(f, res, gamma, beta, scale, eps)
    mag = (f * scale).abs() + res.abs()
    ez = scale * ef + eres + 2 * U * mag                                       # one fma (or a product and a sum)
    emean = ((Lr + 2) * U * mag.sum(1, keepdim=True) + ez.sum(1, keepdim=True)) / n
    d = z - z.mean(1, keepdim=True)
    ed = ez + emean + U * d.abs()
    var = (d * d).mean(1, keepdim=True)
    evar = ((2 * d.abs() * ed + ed * ed).sum(1, keepdim=True) + (Lr + 3) * U * (d * d).sum(1, keepdim=True)) / n
    v = var + eps
    r = rstd.reshape(-1, 1)
    # exact interval of (v +- evar)^-1/2, plus the roundings of eps (fp32), the sum, the square root and the division
    erstd = torch.maximum(torch.clamp(v - evar, min=1e-300) ** -0.5 - r, r - (v + evar) ** -0.5) + 4 * U * r
    exhat = ed * r + d.abs() * erstd + ed * erstd + U * xhat.abs()
    ey = exhat * gamma.abs() + 2 * U * ((xhat * gamma).abs() + beta.abs())
    return {"y": (y, ey), "xhat": (xhat, exhat), "rstd": (rstd, erstd.reshape(-1))}


def ln_bwd(dy, xhat, exhat, rstd, erstd, gamma, scale, ws_rows):
    """reference and bounds of mc_mlp_head_ln_bwd + the ordered sums, given the (xhat, rstd) the kernel is handed and how far
    they are from the reference's (0 at the kernel level): dz, df, dgamma, dbeta, dbias"""
    rows, n = xhat.shape
    Lr = lane_chain(n)
    r, er = rstd.reshape(-1, 1), erstd.reshape(-1, 1)
    g = dy * gamma
    m1 = g.mean(1, keepdim=True)
    m2 = (g * xhat).mean(1, keepdim=True)
    em1 = (Lr + 3) * U * g.abs().sum(1, keepdim=True) / n
    em2 = ((g.abs() * exhat).sum(1, keepdim=True) + (Lr + 4) * U * (g * xhat).abs().sum(1, keepdim=True)) / n
    inner = g - m1 - xhat * m2
    mag = g.abs() + m1.abs() + (xhat * m2).abs()
    einner = U * g.abs() + em1 + xhat.abs() * em2 + exhat * m2.abs() + exhat * em2 + 4 * U * mag
    dz = r * inner
    edz = er * inner.abs() + r * einner + er * einner + U * dz.abs()
    df = dz * scale
    edf = scale * edz + U * df.abs()
    # column sums: a wave adds its rows in sequence, four waves are added through LDS, the fp64 ordered sum rounds once
    Lc = -(-rows // (4 * ws_rows)) + 4 + 1
    out = {"dz": (dz, edz), "df": (df, edf),
           "dgamma": ((dy * xhat).sum(0), (dy.abs() * exhat).sum(0) + (Lc + 2) * U * (dy * xhat).abs().sum(0)),
           "dbeta": (dy.sum(0), (Lc + 1) * U * dy.abs().sum(0)),
           "dbias": (df.sum(0), edf.sum(0) + (Lc + 1) * U * df.abs().sum(0))}
    return out


def module_bounds(x, w, cot, scale, ws_rows, eps=EPS, split_k=False):
    """reference and bounds of one MLPProjectionHead call, forward and backward of sum(out * cot), on exact fp32 operands held
    in fp64: {"out" | "x" | parameter name: (value, bound)}.  The explicit backward is checked against fp64 autograd by the
    tests (head64_grads).  |GELU'| <= 1.13 and |GELU''| <= 0.8 carry the error of p into g and into GELU'(p).  split_k: the two
    forward GEMMs take mc_sgemm's real chain (sgemm_chain) instead of k -- what the model-level bound uses at k = 1408."""
    w1, b1, w2, b2 = w["projection.weight"], w["projection.bias"], w["fc.weight"], w["fc.bias"]
    gamma, beta = w["layer_norm.weight"], w["layer_norm.bias"]
    zero = torch.zeros((), dtype=F64, device=x.device)
    p = x @ w1.T + b1
    m, n = x.shape[0], w1.shape[0]
    ep = gemm_err(x, zero * x, w1.T, zero * w1.T, bias=b1, chain=sgemm_chain(m, n, x.shape[1]) if split_k else None)
    g = gelu64(p)
    eg = 1.13 * ep + gelu_err(p)
    f = g @ w2.T + b2
    ef = gemm_err(g, eg, w2.T, zero * w2.T, bias=b2, chain=sgemm_chain(m, n, n) if split_k else None)
    fw = ln_fwd(f, ef, p, ep, gamma, beta, scale, eps)
    bw = ln_bwd(cot, fw["xhat"][0], fw["xhat"][1], fw["rstd"][0], fw["rstd"][1], gamma, scale, ws_rows)
    (dz, edz), (df, edf) = bw["dz"], bw["df"]
    dw2 = df.T @ g
    edw2 = gemm_err(df.T, edf.T, g, eg)
    dg = df @ w2
    edg = gemm_err(df, edf, w2, zero * w2)
    G = gelu_grad64(p)
    eG = 0.8 * ep + gelu_grad_err(p)
    dp = dg * G + dz
    edp = edg * G.abs() + dg.abs() * eG + edg * eG + edz + 2 * U * ((dg * G).abs() + dz.abs())
    ones = torch.ones((1, x.shape[0]), dtype=F64, device=x.device)
    return {"out": fw["y"], "x": (dp @ w1, gemm_err(dp, edp, w1, zero * w1)),
            "projection.weight": (dp.T @ x, gemm_err(dp.T, edp.T, x, zero * x)),
            "projection.bias": ((ones @ dp).reshape(-1), gemm_err(ones, zero * ones, dp, edp).reshape(-1)),
            "fc.weight": (dw2, edw2), "fc.bias": bw["dbias"],
            "layer_norm.weight": bw["dgamma"], "layer_norm.bias": bw["dbeta"]}
