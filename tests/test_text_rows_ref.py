"""The yardstick of tests/test_text_rows_fp64_gpu.py without a device (tests/_text_rows_ref.py): the fp64 references against torch's
own layer_norm / softmax / gelu through fp64 autograd, an fp32 torch rendition of each kernel formula against every bound (it
must pass), the wrong variants against the same bounds (they must fail, at the stated share of the elements), and the arithmetic
of a softmax row whose keys are all masked."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _text_rows_ref as R

F64, F32, ST, U = R.F64, R.F32, R.ST, R.U
EPS = 1e-12                       # BertConfig.layer_norm_eps
CONTROL_H = (8, 64, 520, 768, 1024)


def close(got, ref, what):
    assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1e-300), what


# ------------------------------------------------------------------------------------------------ references vs torch
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layer_norm_reference_equals_torch_autograd(p):
    rows, h = 11, 72
    x, res = R.ln_inputs("normal", rows, h, 1)
    gamma, beta = R.affine(h, 3)
    keep = R.rows_keep_scale(torch.arange(rows), h, p) if p else None
    dy = R.randn(rows, h, seed=5)
    o = R.add_ln_fwd(x, res, gamma, beta, EPS, keep)
    bw = R.ln_bwd(o, dy)
    xr, rr, gr, br = (t.to(F64).requires_grad_(True) for t in (x, res, gamma, beta))
    y = F.layer_norm((xr * keep if p else xr) + rr, (h,), gr, br, R.eps32(EPS))
    y.backward(dy.to(F64))
    close(o.y, y.detach(), "y")
    s = ((x.to(F64) * keep if p else x.to(F64)) + res.to(F64))
    close(o.mean, s.mean(1), "mean")
    close(o.rstd, (s.var(1, unbiased=False) + R.eps32(EPS)) ** -0.5, "rstd")
    close(bw["dx"][0], xr.grad, "dx")
    close(bw["dres"][0], rr.grad, "dres")
    close(bw["dgamma"][0], gr.grad, "dgamma")
    close(bw["dbeta"][0], br.grad, "dbeta")
    # S of a sum entry is the sum of the |terms|
    close(bw["dbeta"][1], dy.to(F64).abs().sum(0), "S of dbeta")
    assert float(bw["dbeta"][2].min()) == rows


@pytest.mark.parametrize("p,with_tt", [(0.0, True), (0.1, False), (0.1, True)])
def test_embedding_reference_equals_torch_autograd(p, with_tt):
    b, t, h = 3, 16, 64
    cs = R.embed_case(b, t, h, with_tt, 7)
    ids, pos_ids = cs["ids"].reshape(-1), torch.arange(t).repeat(b)
    tt = None if cs["tt"] is None else cs["tt"].reshape(-1)
    gamma, beta = R.affine(h, 11)
    keep = R.rows_keep_scale(torch.arange(b * t), h, p) if p else None
    dy = R.randn(b * t, h, seed=13)
    o = R.embed_fwd(ids, pos_ids, tt, cs["word"], cs["pos"], cs["typ"], gamma, beta, EPS, keep)
    bw = R.ln_bwd(o, dy)
    w, ps, ty, gr, br = (v.to(F64).requires_grad_(True) for v in (cs["word"], cs["pos"], cs["typ"], gamma, beta))
    y = F.layer_norm(w[ids] + ps[pos_ids] + ty[torch.zeros_like(ids) if tt is None else tt], (h,), gr, br, R.eps32(EPS))
    if p:
        y = y * keep
    y.backward(dy.to(F64))
    close(o.y, y.detach(), "y")
    for name, ref in (("dword", w.grad), ("dpos", ps.grad), ("dtype", ty.grad), ("dgamma", gr.grad), ("dbeta", br.grad)):
        close(bw[name][0], ref, name)
    n = bw["dword"][2]
    for u in cs["unused"]:
        assert float(n[u].max()) == 0 and float(bw["dword"][0][u].abs().max()) == 0
    if not p:
        assert float(n[0].min()) >= b * 2 and float(n[1].min()) == b       # id 0: the trailing runs; id 1: every first token


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_softmax_reference_equals_torch_autograd(p):
    rows, t = 7, 40
    s = R.softmax_scores(rows, t, 17, sd=3.0)
    pr, _ = R.softmax_fwd(s)
    sr = s.to(F64).requires_grad_(True)
    ref = torch.softmax(sr, -1)
    close(pr, ref.detach(), "softmax")
    keep = R.keep_scale(rows, t, p, R.SEED, R.SID) if p else None
    dp = R.randn(rows, t, seed=19, dtype=F32)
    ((ref * keep if p else ref) * dp.to(F64)).sum().backward()
    ds, _ = R.softmax_bwd(pr, dp, 0.125, keep)
    close(ds, sr.grad * 0.125, "softmax bwd")


def test_gelu_reference_equals_torch_autograd():
    x = R.randn(4096, seed=23, scale=3.0)
    y, _ = R.gelu_fwd(x)
    xr = x.to(F64).requires_grad_(True)
    ref = F.gelu(xr)
    dy = R.randn(4096, seed=29)
    ref.backward(dy.to(F64))
    # (F.gelu forms 1 + erf: compare where that is not yet a cancelled quantity, and in absolute terms everywhere)
    assert float((y - ref.detach()).abs().max()) <= 1e-15 * float(x.to(F64).abs().max())
    big = x.to(F64) > -1
    close(y[big], ref.detach()[big], "gelu")
    dx, _ = R.gelu_bwd(x, dy)
    close(dx, xr.grad, "gelu bwd")


# ------------------------------------------------------------------------------------------------ fp32 renditions
def ln32(s32, gamma, beta, eps, single_pass=False):
    """the kernel formula in fp32 torch: two-pass variance (single_pass: E[x^2] - mean^2, the control)"""
    h = s32.shape[1]
    m = s32.sum(1) / h
    d = s32 - m[:, None]
    v = (s32 * s32).sum(1) / h - m * m if single_pass else (d * d).sum(1) / h
    r = torch.rsqrt(v + np.float32(eps))
    return m, r, (d * r[:, None]) * gamma + beta


def ln_bwd32(s32, m, r, d, gamma):
    h = s32.shape[1]
    xh = (s32 - m[:, None]) * r[:, None]
    g = d * gamma
    s1 = g.sum(1, keepdim=True) / h
    s2 = (g * xh).sum(1, keepdim=True) / h
    return r[:, None] * (g - s1 - xh * s2), (d * xh).sum(0), d.sum(0)


WORST = {}


def note(name, q):
    """every rendition meets its bound (the 16-bit outputs are dominated by their own rounding and come close to 1)"""
    WORST[name] = max(WORST.get(name, 0.0), q)
    assert q <= 1.0, (name, q)


@pytest.mark.parametrize("kind", ["normal", "offset", "const", "spike"])
@pytest.mark.parametrize("h", [8, 504, 512, 520, 768, 1024])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fp32_add_ln_meets_the_bounds(kind, h, p):
    rows = 37
    x, res = R.ln_inputs(kind, rows, h, 31 + h)
    gamma, beta = R.affine(h, 37)
    keep = R.rows_keep_scale(torch.arange(rows), h, p) if p else None
    dy = R.randn(rows, h, seed=41)
    o = R.add_ln_fwd(x, res, gamma, beta, EPS, keep)
    bw = R.ln_bwd(o, dy)
    k32 = keep.to(F32) if p else None
    s32 = (x.float() * k32 if p else x.float()) + res.float()
    m, r, y = ln32(s32, gamma, beta, EPS)
    note("mean", R.ratio(m, o.mean, o.e_mean))
    note("rstd", R.ratio(r, o.rstd, o.e_rstd))
    note("y", R.ratio(y.to(ST), o.y, o.e_y))
    if kind == "const" and not p:
        assert torch.equal(y.to(ST), beta.to(ST).expand(rows, h)) and torch.equal(m.double(), o.mean)
    dln, dgm, dbt = ln_bwd32(s32, m, r, dy.float(), gamma)
    note("dres", R.ratio(dln.to(ST), *bw["dres"]))
    note("dx", R.ratio((dln * k32 if p else dln).to(ST), *bw["dx"]))
    note("dgamma", R.ratio(dgm, bw["dgamma"][0], R.sum_bound(bw["dgamma"])))
    note("dbeta", R.ratio(dbt, bw["dbeta"][0], R.sum_bound(bw["dbeta"])))


@pytest.mark.parametrize("b,t,h,p", [(3, 16, 64, 0.0), (3, 16, 520, 0.1), (2, 1, 1024, 0.1), (5, 64, 64, 0.1)])
def test_fp32_embedding_meets_the_bounds(b, t, h, p):
    cs = R.embed_case(b, t, h, True, 43)
    ids, pos_ids, tt = cs["ids"].reshape(-1), torch.arange(t).repeat(b), cs["tt"].reshape(-1)
    gamma, beta = R.affine(h, 47)
    keep = R.rows_keep_scale(torch.arange(b * t), h, p) if p else None
    dy = R.randn(b * t, h, seed=53)
    o = R.embed_fwd(ids, pos_ids, tt, cs["word"], cs["pos"], cs["typ"], gamma, beta, EPS, keep)
    bw = R.ln_bwd(o, dy)
    s32 = cs["word"][ids] + cs["typ"][tt] + cs["pos"][pos_ids]
    m, r, y = ln32(s32, gamma, beta, EPS)
    k32 = keep.to(F32) if p else torch.ones_like(y)
    note("embed mean", R.ratio(m, o.mean, o.e_mean))
    note("embed rstd", R.ratio(r, o.rstd, o.e_rstd))
    note("embed y", R.ratio((y * k32).to(ST), o.y, o.e_y))
    dln, dgm, dbt = ln_bwd32(s32, m, r, dy.float() * k32, gamma)
    note("embed dgamma", R.ratio(dgm, bw["dgamma"][0], R.sum_bound(bw["dgamma"])))
    note("embed dbeta", R.ratio(dbt, bw["dbeta"][0], R.sum_bound(bw["dbeta"])))
    for name, idx, n in (("dword", ids, 50), ("dpos", pos_ids, max(t, 2)), ("dtype", tt, 2)):
        got = torch.zeros(n, h).index_add_(0, idx, dln)
        note("embed " + name, R.ratio(got, bw[name][0], R.sum_bound(bw[name])))


@pytest.mark.parametrize("t", [1, 8, 24, 40, 100, 511, 16, 64, 512])
@pytest.mark.parametrize("sd,offset", [(1.0, 0.0), (3.0, 0.0), (20.0, 0.0), (1.0, 1e4)])
def test_fp32_softmax_meets_the_bounds(t, sd, offset):
    rows = 33
    s = R.softmax_scores(rows, t, 59 + t, sd=sd, offset=offset)
    pr, bound = R.softmax_fwd(s)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    p32 = e * (1.0 / e.sum(1, keepdim=True))
    note("softmax", R.ratio(p32.to(ST), pr, bound))
    assert torch.equal(p32[-1].to(ST), torch.full((t,), 1.0 / t).to(ST)) and float(p32[-2, t // 2]) == 1.0
    keep = R.keep_scale(rows, t, 0.5, R.SEED, R.SID) if t % 8 == 0 else None
    dp = R.randn(rows, t, seed=61, dtype=F32)
    ds, dbound = R.softmax_bwd(p32.to(ST), dp, 0.125, keep)
    p16, d32 = p32.to(ST).float(), dp if keep is None else dp * keep.float()
    got = p16 * (d32 - (p16 * d32).sum(1, keepdim=True)) * 0.125
    note("softmax bwd", R.ratio(got.to(ST), ds, dbound))


def test_fp32_gelu_meets_the_bounds_on_every_pattern():
    x = R.all_finite_patterns()
    assert x.numel() % 8 == 0 and x.numel() > (65000 if ST == torch.bfloat16 else 61000)
    xf = x.float()
    y, bound = R.gelu_fwd(x)
    note("gelu", R.ratio((0.5 * xf * (1.0 + torch.erf(xf * np.float32(0.70710678118654752)))).to(ST), y, bound))
    g32 = 0.5 * (1.0 + torch.erf(xf * np.float32(0.70710678118654752))) + xf * (np.float32(0.39894228040143268) * torch.exp(-0.5 * xf * xf))
    for dy in (torch.ones_like(x), R.randn(x.numel(), seed=67)):
        dx, dbound = R.gelu_bwd(x, dy)
        assert torch.isfinite(dx).all() and torch.isfinite(g32).all()
        note("gelu bwd", R.ratio((dy.float() * g32).to(ST), dx, dbound))
    # the far tail: the reference's derivative is 0 resp. 1 where x * x overflows fp32
    far = xf.abs() > 1e20
    assert (far.any() or ST != torch.bfloat16) and torch.equal(R.gelu_grad(x)[0][far], (xf[far] > 0).double())


# ------------------------------------------------------------------------------------------------ controls
@pytest.mark.parametrize("h", CONTROL_H)
def test_control_single_pass_variance_violates_rstd_and_y(h):
    rows = 37
    x, res = R.ln_inputs("offset", rows, h, 71 + h)
    gamma, beta = R.affine(h, 73)
    o = R.add_ln_fwd(x, res, gamma, beta, EPS)
    assert float((o.mean - 64).abs().max()) < 1.0 and 0.02 < float(o.var.min()) and float(o.var.max()) < 0.8
    s32 = x.float() + res.float()
    m, r, y = ln32(s32, gamma, beta, EPS, single_pass=True)
    rel = (r.double() - o.rstd).abs() / o.rstd
    assert bool(((r.double() - o.rstd).abs() > o.e_rstd).all()), (h, float(rel.min()), float(o.e_rstd_rel.max()))
    share = R.violations(y.to(ST), o.y, o.e_y)
    print(f"h {h}: single-pass rstd rel err {float(rel.min()):.2e} .. {float(rel.max()):.2e}, bound {float(o.e_rstd_rel.min()):.2e} .. "
          f"{float(o.e_rstd_rel.max()):.2e}, y share {share:.3f}")
    assert share >= 0.02, (h, share)
    # the two-pass form on the same rows is far inside
    _, r2, _ = ln32(s32, gamma, beta, EPS)
    assert R.ratio(r2, o.rstd, o.e_rstd) <= 0.25


@pytest.mark.parametrize("t", [8, 40, 100, 512])
def test_control_softmax_without_the_last_key_in_the_sum(t):
    s = R.randn(33, t, seed=79 + t, dtype=F32)
    pr, bound = R.softmax_fwd(s)
    e = torch.exp(s.double() - s.double().max(1, keepdim=True).values)
    wrong = e / (e.sum(1, keepdim=True) - e[:, -1:])
    share = R.violations(wrong.to(ST), pr, bound)
    print(f"t {t}: share {share:.3f}")
    assert share >= 0.10, (t, share)


def test_control_tanh_gelu():
    x = R.all_finite_patterns()
    x = x[(x.float().abs() >= 2.0 ** -6) & (x.float().abs() <= 8)]
    y, bound = R.gelu_fwd(x)
    xd = x.double()
    wrong = 0.5 * xd * (1 + torch.tanh(math.sqrt(2 / math.pi) * (xd + 0.044715 * xd ** 3)))
    share = R.violations(wrong.to(ST), y, bound)
    print(f"tanh GELU: share {share:.3f} of {x.numel()} patterns")
    assert share >= 0.05, share


def last_term(terms, index, n_index):
    """[n_index, h]: the term of the LAST row that contributes to each entry (0 where none does)"""
    out = torch.zeros(n_index, terms.shape[1], dtype=F64)
    for r in range(terms.shape[0]):
        i = int(index[r])
        out[i] = torch.where(terms[r] != 0, terms[r], out[i])
    return out


def test_control_sum_with_one_row_dropped():
    rows, h = 37, 64
    x, res = R.ln_inputs("normal", rows, h, 83)
    gamma, beta = R.affine(h, 89)
    dy = R.randn(rows, h, seed=97)
    o = R.add_ln_fwd(x, res, gamma, beta, EPS)
    bw = R.ln_bwd(o, dy)
    shares = {}
    zero = torch.zeros(rows, dtype=torch.int64)
    for name, terms in (("dgamma", dy.double() * o.xhat), ("dbeta", dy.double())):
        shares["add_ln " + name] = float((last_term(terms, zero, 1)[0].abs() > R.sum_bound(bw[name])).double().mean())
    b, t = 3, 16
    cs = R.embed_case(b, t, h, True, 101)
    ids, pos_ids, tt = cs["ids"].reshape(-1), torch.arange(t).repeat(b), cs["tt"].reshape(-1)
    e = R.embed_fwd(ids, pos_ids, tt, cs["word"], cs["pos"], cs["typ"], gamma, beta, EPS)
    ebw = R.ln_bwd(e, R.randn(b * t, h, seed=103))
    dln = ebw["dln"][0]
    for name, idx, n in (("dword", ids, 50), ("dpos", pos_ids, t), ("dtype", tt, 2)):
        named = ebw[name][2] > 0
        bad = last_term(dln, idx, ebw[name][0].shape[0]).abs() > R.sum_bound(ebw[name])
        shares["embed " + name] = float(bad[named].double().mean())
    print({k: round(v, 3) for k, v in shares.items()})
    assert min(shares.values()) >= 0.80, shares


# ------------------------------------------------------------------------------------------------ the fully masked row
def general_body(row, start):
    """softmax_fwd_k's arithmetic on one fp32 row: running maximum from `start`, exp(s - max), 1 / sum, product"""
    with np.errstate(divide="ignore", invalid="ignore"):
        mx = np.maximum(np.float32(start), row.max())
        e = np.exp(row - mx, dtype=np.float32)
        return e * (np.float32(1) / e.sum(dtype=np.float32))


@pytest.mark.parametrize("t", [1, 8, 40, 100, 511])
def test_fully_masked_row_is_uniform(t):
    s = torch.full((1, t), R.NEG, dtype=F32)
    assert float(s[0, 0]) == torch.finfo(F32).min
    pr, bound = R.softmax_fwd(s)
    assert torch.equal(pr, torch.full((1, t), 1.0 / t, dtype=F64))
    assert torch.equal(torch.softmax(s, -1), torch.full((1, t), 1.0 / t))
    row = s[0].numpy()
    assert np.isnan(general_body(row, -3.4e38)).all()               # the initial maximum before the fix lies ABOVE the mask bias
    fixed = general_body(row, -np.inf)
    assert (fixed == np.float32(1) / np.float32(t)).all()
    assert R.ratio(torch.from_numpy(fixed).to(ST)[None], pr, bound) <= 1.0
    # a row of -inf stays NaN, as in torch
    assert np.isnan(general_body(np.full(t, -np.inf, dtype=np.float32), -np.inf)).all()
    assert torch.isnan(torch.softmax(torch.full((1, t), -math.inf), -1)).all()


def test_zz_print_worst_rendition_ratios():
    print({k: round(v, 3) for k, v in sorted(WORST.items())})
