"""Op-level parity of every HIP kernel (through the C ABI) against plain PyTorch fp32 references of the
same op, on seeded inputs.  GPU only (`pytest -m gpu`).

Tolerances: kernels compute in fp32 from bf16 operands and round the result once to bf16, so the bound is
bf16 round-off: max-abs error <= 1e-2 * max|ref| (2^-8 = 3.9e-3 per rounding) unless noted; fp32-in/fp32-out
kernels are held to 1e-4.  For the GEMM kernels that bound is global: an error confined to one output tile -- one lost
reduction element, a K tail one chunk short, an unwritten last row of a ragged tile, a write outside the tile -- stays under
1e-2 * max|ref| of a Gaussian product.  tests/test_gemm_exact_gpu.py runs the same kernels on +-1 operands, where the product
is exact and compared with torch.equal, inside guarded buffers, at the smallest shapes that reach each path.

Launchers with a capped grid (the row, element, cast and column-sum kernels) run their later passes only past a
row / element count; the `*_past_the_grid_cap` tests cross each cap by one ragged workgroup, with fp64 references:
    per-row / per-element output   check_late(): `check` on the whole tensor AND on the slice past the first pass,
                                   so the later passes are normalised by their own max|ref|
    sums over rows (dgamma, ...)   a second call whose input is zero in the rows of the first pass: the sum then comes
                                   from the later passes alone and is compared with the fp64 sum of those rows
max|ref| of the whole tensor is not enough for a capped reduction: a sum over 2053 rows that lost its last 5 rows moves
by ~1.6 % of max|ref| and, with more rows, falls under any bound that a complete sum is held to.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16               # the 16-bit storage dtype of the loaded kernel library (bf16; f16 under MC_STORAGE=f16)


@pytest.fixture(autouse=True)
def _kernel_switches_on():
    """the kernels are tested whatever the developer A/B switches of the environment say (MC_XDW / MC_EFREE = 0)"""
    old = ops.XDW, ops.EFREE
    ops.XDW, ops.EFREE = 1, 1
    yield
    ops.XDW, ops.EFREE = old


def rnd(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def relerr(got, ref):
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def check(got, ref, tol, what=""):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got.float()).all(), what + ": non-finite"
    e = relerr(got, ref)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol}"


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(300, 144, 24), (1000, 24, 144), (257, 40, 240), (129, 1408, 352),
                                   (512, 768, 768), (77, 16, 16), (4096, 304, 1824), (130, 64, 48)])
def test_gemm_nt(M, N, K):
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    y = ops.linear_fwd(x, w)
    check(y, x.float() @ w.float().T, 1e-2, "nt")


def test_gemm_nt_asymmetric_identity():
    # A = I catches an output transpose (cdna guide: always test with asymmetric B)
    n = 128
    a = torch.eye(n, device=DEV).to(BF)
    b = (torch.arange(n * n, device=DEV).reshape(n, n) % 61).float().to(BF)
    y = ops.linear_fwd(a, b)
    check(y, b.float().T, 1e-6, "identity")


def test_gemm_bias_gelu_residual_stats():
    M, N, K = 700, 3072, 768
    x, w = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=K ** -0.5)
    bias = rnd(N, seed=5, dtype=torch.float32)
    y = ops.gelu_fwd(ops.linear_fwd(x, w, bias=bias))
    check(y, F.gelu((x.float() @ w.float().T + bias).to(BF).float()), 1e-2, "bias, then gelu")
    res = rnd(M, 768, seed=6)
    w2 = rnd(768, N, seed=7, scale=N ** -0.5)
    y2 = ops.linear_fwd(y, w2, bias=bias[:768].contiguous(), residual=res)
    ref2 = (y.float() @ w2.float().T + bias[:768]).to(BF).float() + res.float()
    check(y2, ref2, 1e-2, "residual")
    y3, part = ops.linear_fwd(x, w, stats=True)
    s = part.double().sum(0)
    yf = y3.float().double()
    check(s[0].float(), yf.sum(0).float(), 1e-4, "colsum")
    check(s[1].float(), (yf * yf).sum(0).float(), 1e-4, "colsumsq")


@pytest.mark.parametrize("M,N,K", [(300, 24, 144), (1000, 240, 40), (513, 352, 1408), (64, 768, 3072)])
def test_gemm_dgrad_nn(M, N, K):
    dy, w = rnd(M, N, seed=8), rnd(N, K, seed=9, scale=N ** -0.5)
    res = rnd(M, K, seed=10)
    dx = ops.linear_dgrad(dy, w, residual=res)
    ref = (dy.float() @ w.float()).to(BF).float() + res.float()
    check(dx, ref, 1e-2, "dgrad")


@pytest.mark.parametrize("M,N,K", [(5000, 144, 24), (3000, 24, 144), (70000, 240, 40), (1392, 1824, 304), (999, 48, 32)])
def test_gemm_wgrad_tn(M, N, K):
    dy, x = rnd(M, N, seed=11), rnd(M, K, seed=12)
    dw = ops.linear_wgrad(dy, x)
    check(dw, dy.float().T @ x.float(), 2e-3, "wgrad")


class _force_gemm256_tn:
    """MC_GEMM_256TN for the launches inside: 2 = the 256 x 256 TN kernel whenever the layout allows, 0 = never"""

    def __init__(self, mode="2"):
        self.mode = mode

    def __enter__(self):
        self.old = os.environ.get("MC_GEMM_256TN")
        os.environ["MC_GEMM_256TN"] = self.mode

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("MC_GEMM_256TN", None)
        else:
            os.environ["MC_GEMM_256TN"] = self.old


@pytest.mark.parametrize("M,N,K", [(4096, 304, 1824), (44544, 1824, 304), (5000, 176, 1056), (16384, 768, 3072), (3000, 264, 40),
                                   (700, 256, 256), (64, 8, 8)])
def test_gemm256_tn_wgrad(M, N, K):
    """256 x 256 x 64 transpose-read TN kernel (gemm256_tn.hip): dW = dY^T X, split-K through the workspace (plan from
    mc_gemm256_tn_splits), ragged output tiles, K ranges that end inside a K tile, accumulation into an existing dW, and
    the production route (rule-based eligibility) giving the same result."""
    dy, x = rnd(M, N, seed=11), rnd(M, K, seed=12)
    ref = dy.float().T @ x.float()
    with _force_gemm256_tn():
        assert ops._tn256_plan(N, K, M, N, K) >= 1
        dw = ops.linear_wgrad(dy, x)
        check(dw, ref, 2e-3, "gemm256_tn wgrad")
        if not L.load().mc_wgrad_rows_supported(N, K):
            dw2 = ops.linear_wgrad(dy, x, out=dw.clone())
            check(dw2, 2 * ref, 2e-3, "gemm256_tn wgrad accumulate")
    check(ops.linear_wgrad(dy, x), ref, 2e-3, "wgrad (default route)")


@pytest.mark.parametrize("n_img,hw,N,K", [(4, 1392, 304, 1824), (3, 5415, 176, 1056), (5, 700, 512, 3072)])
def test_gemm256_tn_grouped_gate(n_img, hw, N, K):
    """grouped split-K on the TN tile kernel: reduction cut at image boundaries, the SE gate applied to each image's
    partial when the partials are combined [ref: efficientnet_custom.py:114-122 backward]"""
    M = n_img * hw
    x, dy = rnd(M, K, seed=101), rnd(M, N, seed=104)
    gate = torch.sigmoid(rnd(n_img, K, seed=103, dtype=torch.float32))
    img = torch.arange(M, device=DEV) // hw
    ref = dy.float().T @ (x.float() * gate[img])
    with _force_gemm256_tn():
        assert ops._tn256_plan(N, K, M, N, K, group_rows=hw) >= 1
        dw = ops.linear_wgrad(dy, x, pro=(None, None, gate, hw))
    check(dw, ref, 3e-3, "gemm256_tn grouped gate wgrad")


@pytest.mark.parametrize("route", ["0", "2"])
@pytest.mark.parametrize("M,N", [(136, 264), (40, 24)])
def test_gemm_tn_empty_split(M, N, route):
    """a split whose K range is empty still owes its (zero) partial tile: 9 K tiles of 64 rows over 4 splits give 3 tiles
    per split, so split 3 starts at row 576 = K.  The workspace starts as NaN: a partial tile that is not written shows in
    the sum.  Route 0 = the 128-row tile family (136 x 264: ragged direct-to-LDS tiles, 40 x 24: register-staged narrow
    tiles), route 2 = the 256 x 256 TN kernel."""
    K, splits = 576, 4
    a, b = rnd(K, M, seed=21), rnd(K, N, seed=22)
    ws = torch.full((splits, M, N), float("nan"), device=DEV, dtype=torch.float32)
    c = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32)
    with _force_gemm256_tn(route):
        ops.gemm(a, b, c, M, N, K, M, N, N, a_kmajor=1, b_kmajor=1, c_f32=1, splits=splits, splitk_ws=ws)
    check(c, a.float().T @ b.float(), 2e-3, f"tn empty split, route {route}")


def test_gemm_prologue_a_and_b():
    n_img, hw, Cc, N = 3, 50, 144, 24
    M = n_img * hw
    d = rnd(M, Cc, seed=13)
    scale, shift = rnd(Cc, seed=14, dtype=torch.float32) * 0.5 + 1.0, rnd(Cc, seed=15, dtype=torch.float32) * 0.3
    gate = torch.sigmoid(rnd(n_img, Cc, seed=16, dtype=torch.float32))
    w = rnd(N, Cc, seed=17, scale=Cc ** -0.5)
    a1 = (F.silu(d.float() * scale + shift).view(n_img, hw, Cc) * gate[:, None, :]).view(M, Cc).to(BF).float()
    y = ops.linear_fwd(d, w, pro=(scale, shift, gate, hw))
    check(y, a1 @ w.float().T, 1e-2, "prologue A")
    dy = rnd(M, N, seed=18)
    dw = ops.linear_wgrad(dy, d, pro=(scale, shift, gate, hw))
    check(dw, dy.float().T @ a1, 2e-3, "prologue B")
    y2 = ops.linear_fwd(d, w, pro=(scale, shift, None, hw))
    check(y2, F.silu(d.float() * scale + shift).to(BF).float() @ w.float().T, 1e-2, "prologue A no gate")


class _force_gemm256:
    """route every layout-eligible launch to the 256 x 256 tile kernel (MC_GEMM_256=2), whatever its size"""

    def __enter__(self):
        import os
        self.old = os.environ.get("MC_GEMM_256")
        os.environ["MC_GEMM_256"] = "2"

    def __exit__(self, *a):
        import os
        if self.old is None:
            os.environ.pop("MC_GEMM_256", None)
        else:
            os.environ["MC_GEMM_256"] = self.old


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (512, 256, 128), (300, 144, 24), (257, 40, 240), (4096, 304, 1824),
                                   (5000, 1824, 304), (1392 * 3, 512, 3072), (8192, 2304, 768), (777, 776, 1000),
                                   (66000, 176, 1056), (130, 64, 48), (20000, 3072, 512)])
def test_gemm256_nt(M, N, K):
    """256 x 256 x 64 tile kernel (gemm256.hip): ragged M / N / K tails, one to many K tiles per output tile, more
    output tiles than workgroups (persistent stream across tiles), every path of the staged pipeline; 3 repeats on
    fresh outputs (a race between the DMA stream and the fragment reads would come and go)."""
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    ref = x.float() @ w.float().T
    with _force_gemm256():
        for rep in range(3):
            y = ops.linear_fwd(x, w)
            check(y, ref, 1e-2, f"gemm256 nt rep {rep}")
    # asymmetric identity: catches transposed / permuted fragments exactly
    n = 512
    a = torch.eye(n, device=DEV).to(BF)
    b = (torch.arange(n * n, device=DEV).reshape(n, n) % 61).float().to(BF)
    with _force_gemm256():
        y = ops.linear_fwd(a, b)
    check(y, b.float().T, 1e-6, "gemm256 identity")


def test_gemm256_bias_residual_stats_batched_alpha():
    M, N, K = 3000, 1000, 712
    x, w = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=K ** -0.5)
    bias = rnd(N, seed=5, dtype=torch.float32)
    res = rnd(M, N, seed=6)
    with _force_gemm256():
        y = ops.linear_fwd(x, w, bias=bias, residual=res)
        y3, part = ops.linear_fwd(x, w, stats=True)
    check(y, (x.float() @ w.float().T + bias).to(BF).float() + res.float(), 1e-2, "gemm256 bias+residual")
    assert part.shape == ((M + 255) // 256, 2, N)
    s = part.double().sum(0)
    yf = y3.float().double()
    check(s[0].float(), yf.sum(0).float(), 1e-4, "gemm256 colsum")
    check(s[1].float(), (yf * yf).sum(0).float(), 1e-4, "gemm256 colsumsq")
    # batched (one weight matrix per batch element, like the per-image gated projection weights) + alpha + stats
    nb, hw, N2, K2 = 5, 700, 304, 1824
    xb, wb = rnd(nb * hw, K2, seed=7), rnd(nb, N2, K2, seed=8, scale=K2 ** -0.5)
    yb = torch.empty(nb * hw, N2, device=DEV, dtype=BF)
    with _force_gemm256():
        pb = ops.gemm(xb, wb, yb, hw, N2, K2, K2, K2, N2, batch=nb, sA=(hw * K2, 0), sB=(N2 * K2, 0), sC=(hw * N2, 0),
                      alpha=0.5, stats=True)
    refb = 0.5 * torch.einsum("bmk,bnk->bmn", xb.float().view(nb, hw, K2), wb.float()).reshape(nb * hw, N2)
    check(yb, refb, 1e-2, "gemm256 batched")
    assert pb.shape == (nb * ((hw + 255) // 256), 2, N2)
    check(pb.double().sum(0)[0].float(), yb.float().double().sum(0).float(), 1e-4, "gemm256 batched colsum")
    # strided output / operands (columns of a wider buffer, like the fused QKV projection)
    H = 768
    xs = rnd(2048, 3 * H, seed=9)
    ws = rnd(H, H, seed=10, scale=H ** -0.5)
    out = torch.zeros(2048, 3 * H, device=DEV, dtype=BF)
    with _force_gemm256():
        ops.gemm(xs[:, H:], ws, out[:, 2 * H:], 2048, H, H, 3 * H, H, 3 * H)
    check(out[:, 2 * H:], xs[:, H:2 * H].float() @ ws.float().T, 1e-2, "gemm256 strided")
    assert float(out[:, :2 * H].abs().max()) == 0.0


def test_gemm_batched_attention_shapes():
    b, nh, T, hd = 2, 3, 64, 64
    H = nh * hd
    qkv = rnd(b * T, 3 * H, seed=19)
    maskb = torch.zeros(b, T, device=DEV)
    maskb[1, 40:] = -3.0e38
    scores = torch.empty(b, nh, T, T, device=DEV, dtype=torch.float32)
    ops.gemm(qkv, qkv[:, H:], scores, T, T, hd, 3 * H, 3 * H, T, c_f32=1, batch=b * nh, nb2=nh,
             sA=(T * 3 * H, hd), sB=(T * 3 * H, hd), sC=(nh * T * T, T * T), bias=maskb, bias_stride1=T, alpha=0.125)
    q = qkv[:, :H].float().view(b, T, nh, hd).permute(0, 2, 1, 3)
    k = qkv[:, H:2 * H].float().view(b, T, nh, hd).permute(0, 2, 1, 3)
    v = qkv[:, 2 * H:].float().view(b, T, nh, hd).permute(0, 2, 1, 3)
    ref = q @ k.transpose(-1, -2) * 0.125 + maskb[:, None, None, :]
    check(scores.clamp_min(-1e4), ref.clamp_min(-1e4), 1e-4, "qk^T")
    assert float(scores[1, :, :, 40:].max()) < -1e37
    probs = torch.softmax(ref, -1).to(BF)
    ctx = torch.empty(b * T, H, device=DEV, dtype=BF)
    ops.gemm(probs, qkv[:, 2 * H:], ctx, T, hd, T, T, 3 * H, H, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * T * T, T * T), sB=(T * 3 * H, hd), sC=(T * H, hd))
    refctx = (probs.float() @ v).permute(0, 2, 1, 3).reshape(b * T, H)
    check(ctx, refctx, 1e-2, "pv")
    # dV = P^T dO  (a_kmajor + b_kmajor), written into the v-columns of a [b*T, 3H] buffer
    do = rnd(b * T, H, seed=20)
    dqkv = torch.zeros(b * T, 3 * H, device=DEV, dtype=BF)
    ops.gemm(probs, do, dqkv[:, 2 * H:], T, hd, T, T, H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * T * T, T * T), sB=(T * H, hd), sC=(T * 3 * H, hd))
    dov = do.float().view(b, T, nh, hd).permute(0, 2, 1, 3)
    refdv = (probs.float().transpose(-1, -2) @ dov).permute(0, 2, 1, 3).reshape(b * T, H)
    check(dqkv[:, 2 * H:], refdv, 1e-2, "dv")
    assert float(dqkv[:, :2 * H].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K", [(10000, 144, 24), (9001, 24, 48), (20000, 240, 40), (8200, 40, 240), (8192, 64, 384),
                                   (30000, 16, 16), (12345, 64, 384), (9000, 96, 16),
                                   (9000, 768, 128), (10001, 1056, 176), (8300, 264, 40)])   # wide outputs: 128-column tiles
def test_gemm_rows_streaming(M, N, K):
    """row-streaming kernel (full-row ownership, LDS-resident weights): fwd with stats + residual, prologue, dgrad"""
    x, w = rnd(M, K, seed=82), rnd(N, K, seed=83, scale=K ** -0.5)
    res = rnd(M, N, seed=84)
    assert ops._rows_ok(M, N, K, None, 0)
    y, part = ops.linear_fwd(x, w, stats=True)
    ref = x.float() @ w.float().T
    check(y, ref, 1e-2, "rows fwd")
    st = part.double().sum(0)
    yf = y.float().double()
    check(st[0].float(), yf.sum(0).float(), 1e-4, "rows colsum")
    check(st[1].float(), (yf * yf).sum(0).float(), 1e-4, "rows colsumsq")
    y2 = ops.linear_fwd(x, w, residual=res)
    check(y2, ref.to(BF).float() + res.float(), 1e-2, "rows residual")
    hw = 1000
    n_img = (M + hw - 1) // hw
    scale, shift = rnd(K, seed=85, dtype=torch.float32) * 0.5 + 1.0, rnd(K, seed=86, dtype=torch.float32) * 0.3
    gate = torch.sigmoid(rnd(n_img, K, seed=87, dtype=torch.float32))
    img = torch.arange(M, device=DEV) // hw
    a1 = (F.silu(x.float() * scale + shift) * gate[img]).to(BF).float()
    y3 = ops.linear_fwd(x, w, pro=(scale, shift, gate, hw))
    check(y3, a1 @ w.float().T, 1e-2, "rows prologue")
    # data gradient through the transposed weight: dx[M,K] = dy[M,N] . w[N,K]
    dy = rnd(M, N, seed=88)
    wf32 = w.float()
    if ops._rows_ok(M, K, N, None, 0):
        dx = ops.linear_dgrad(dy, w, w_t=ops.cast_transpose_bf16(wf32))
        check(dx, dy.float() @ wf32, 1e-2, "rows dgrad")


@pytest.mark.parametrize("M,N,K", [(10000, 144, 24), (9001, 24, 48), (20000, 240, 40), (8200, 40, 240), (8192, 64, 384),
                                   (30000, 24, 24), (12345, 384, 64), (9000, 16, 96), (70001, 240, 64)])
def test_wgrad_rows_streaming(M, N, K):
    """streaming weight gradient (LDS transpose-reads): plain, with BN+SiLU+gate prologue on X, accumulate"""
    import mammo_clip_amd.lib as L
    assert L.load().mc_wgrad_rows_supported(N, K)
    dy, x = rnd(M, N, seed=89), rnd(M, K, seed=90)
    ref = dy.float().T @ x.float()
    dw = ops.linear_wgrad(dy, x)
    check(dw, ref, 2e-3, "wgrad rows")
    dw2 = ops.linear_wgrad(dy, x, out=dw.clone())
    check(dw2, 2 * ref, 2e-3, "wgrad rows accumulate")
    hw = 777
    n_img = (M + hw - 1) // hw
    scale, shift = rnd(K, seed=91, dtype=torch.float32) * 0.5 + 1.0, rnd(K, seed=92, dtype=torch.float32) * 0.3
    gate = torch.sigmoid(rnd(n_img, K, seed=93, dtype=torch.float32))
    img = torch.arange(M, device=DEV) // hw
    a1 = (F.silu(x.float() * scale + shift) * gate[img]).to(BF).float()
    dw3 = ops.linear_wgrad(dy, x, pro=(scale, shift, gate, hw))
    check(dw3, dy.float().T @ a1, 2e-3, "wgrad rows prologue")


@pytest.mark.parametrize("n_img,hw,N,K", [(4, 300, 176, 1056), (3, 1392, 304, 1824), (8, 256, 40, 768)])
def test_gate_only_project_paths(n_img, hw, N, K):
    """late-stage project conv on an already activated input: forward = one GEMM per image with the weight tile scaled by
    that image's SE gate (+ BN statistics across the batch); weight gradient = split-K cut at image boundaries with the
    gate applied when the partials are combined"""
    M = n_img * hw
    x, w = rnd(M, K, seed=101), rnd(N, K, seed=102, scale=K ** -0.5)
    gate = torch.sigmoid(rnd(n_img, K, seed=103, dtype=torch.float32))
    img = torch.arange(M, device=DEV) // hw
    xg = x.float() * gate[img]
    y, part = ops.linear_fwd(x, w, stats=True, pro=(None, None, gate, hw))
    # the gate is folded into the bf16 weight tile: compare against gate-scaled, bf16-rounded weights per image
    ref = torch.cat([x[i * hw:(i + 1) * hw].float() @ (w.float() * gate[i]).to(BF).float().T for i in range(n_img)])
    check(y, ref, 1e-2, "gate-only fwd")
    st = part.double().sum(0)
    yf = y.float().double()
    check(st[0].float(), yf.sum(0).float(), 1e-4, "gate-only colsum")
    check(st[1].float(), (yf * yf).sum(0).float(), 1e-4, "gate-only colsumsq")
    dy = rnd(M, N, seed=104)
    dw = ops.linear_wgrad(dy, x, pro=(None, None, gate, hw))
    check(dw, dy.float().T @ xg, 3e-3, "gate-only wgrad")


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("nhwc_view", [False, True])
def test_stem_im2col_gemm(nhwc_view):
    n, h, w, c0 = 2, 37, 30, 48
    g = torch.Generator().manual_seed(21)
    if nhwc_view:
        x = torch.randn(n, h, w, 3, generator=g).to(DEV).permute(0, 3, 1, 2)   # trainer_ddp.py:288-291
    else:
        x = torch.randn(n, 3, h, w, generator=g).to(DEV)
    wt = rnd(c0, 3, 3, 3, seed=22, dtype=torch.float32)
    pad = (0, 1, 0, 1)
    oh, ow = (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1
    patches = ops.stem_im2col(x, pad[0], pad[2], oh, ow)
    wb = ops.stem_weight_prep(wt)
    y = ops.linear_fwd(patches, wb)
    ref = F.conv2d(F.pad(x.to(BF).float(), pad), wt.to(BF).float(), None, 2)
    check(y.view(n, oh, ow, c0).permute(0, 3, 1, 2), ref, 1e-2, "stem")


# ------------------------------------------------------------------------------------------------ depthwise
DW_CASES = [(3, 1, (1, 1, 1, 1), 2, 19, 23, 48), (5, 1, (2, 2, 2, 2), 2, 17, 9, 240), (3, 2, (0, 1, 0, 1), 2, 20, 18, 144),
            (5, 2, (1, 2, 1, 2), 1, 21, 19, 40), (3, 2, (1, 1, 1, 1), 2, 9, 9, 72), (5, 2, (2, 2, 2, 2), 1, 15, 15, 16),
            (5, 1, (2, 2, 2, 2), 1, 40, 33, 16), (3, 1, (1, 1, 1, 1), 2, 37, 41, 240), (3, 2, (0, 1, 0, 1), 1, 26, 21, 240)]


def _dw_ref(x_nhwc, w, k, s, pad, pro):
    n, h, wd, c = x_nhwc.shape
    xin = x_nhwc.float()
    if pro is not None:
        xin = F.silu(xin * pro[0] + pro[1]).to(BF).float()
    xin = xin.permute(0, 3, 1, 2)
    return F.conv2d(F.pad(xin, pad), w, None, s, 0, 1, c)


@pytest.mark.parametrize("k,s,pad,n,h,w,c", DW_CASES)
@pytest.mark.parametrize("use_pro", [False, True])
def test_dwconv_fwd(k, s, pad, n, h, w, c, use_pro):
    x = rnd(n, h, w, c, seed=23)
    wt = rnd(c, 1, k, k, seed=24, dtype=torch.float32) * 0.3
    pro = None
    if use_pro:
        pro = (rnd(c, seed=25, dtype=torch.float32) * 0.3 + 1.0, rnd(c, seed=26, dtype=torch.float32) * 0.3)
    ref = _dw_ref(x, wt, k, s, pad, pro)
    oh, ow = ref.shape[2], ref.shape[3]
    w_kkc = wt.view(c, k * k).t().contiguous()
    y, part = ops.dwconv_fwd(x.view(-1, c), w_kkc, n, h, w, c, k, s, pad[0], pad[2], oh, ow, pro=pro, stats=True)
    check(y.view(n, oh, ow, c).permute(0, 3, 1, 2), ref, 1e-2, "dw fwd")
    st = part.double().sum(0)
    yf = y.float().double()
    check(st[0].float(), yf.sum(0).float(), 1e-4, "dw colsum")
    check(st[1].float(), (yf * yf).sum(0).float(), 1e-4, "dw colsumsq")


@pytest.mark.parametrize("k,s,pad,n,h,w,c", DW_CASES)
def test_dwconv_bwd(k, s, pad, n, h, w, c):
    x = rnd(n, h, w, c, seed=27)
    wt = rnd(c, 1, k, k, seed=28, dtype=torch.float32) * 0.3
    pro = (rnd(c, seed=29, dtype=torch.float32) * 0.3 + 1.0, rnd(c, seed=30, dtype=torch.float32) * 0.3)
    a = F.silu(x.float() * pro[0] + pro[1]).to(BF).float().permute(0, 3, 1, 2).requires_grad_(True)
    wr = wt.clone().requires_grad_(True)
    y = F.conv2d(F.pad(a, pad), wr, None, s, 0, 1, c)
    oh, ow = y.shape[2], y.shape[3]
    dy = rnd(n, oh, ow, c, seed=31)
    y.backward(dy.float().permute(0, 3, 1, 2))
    w_kkc = wt.view(c, k * k).t().contiguous()
    w_flip = wt.flip(2, 3).reshape(c, k * k).t().contiguous()
    dx = ops.dwconv_bwd_data(dy.view(-1, c), w_kkc, n, h, w, c, k, s, pad[0], pad[2], oh, ow)
    check(dx.view(n, h, w, c).permute(0, 3, 1, 2), a.grad, 1e-2, "dw bwd data (gather)")
    if s == 1:
        dx2 = ops.dwconv_bwd_data(dy.view(-1, c), w_kkc, n, h, w, c, k, s, pad[0], pad[2], oh, ow, w_kkc_flipped=w_flip)
        check(dx2.view(n, h, w, c).permute(0, 3, 1, 2), a.grad, 1e-2, "dw bwd data (flipped fwd)")
    dw = ops.dwconv_bwd_weight(x.view(-1, c), dy.view(-1, c), n, h, w, c, k, s, pad[0], pad[2], oh, ow, pro=pro)
    check(dw.t().reshape(c, 1, k, k), wr.grad, 2e-3, "dw bwd weight")


# ------------------------------------------------------------------------------------------------ BN family
@pytest.mark.parametrize("n_img,hw,c", [(3, 50, 48), (2, 333, 240), (4, 9, 3072), (1, 1000, 16)])
def test_bn_train_fwd_bwd(n_img, hw, c):
    M = n_img * hw
    x = rnd(M, c, seed=32) * 1.5 + 0.3
    gamma = rnd(c, seed=33, dtype=torch.float32) * 0.2 + 1.0
    beta = rnd(c, seed=34, dtype=torch.float32) * 0.2
    rm0, rv0 = rnd(c, seed=35, dtype=torch.float32) * 0.1, torch.rand(c, device=DEV) + 0.5
    # statistics via the GEMM epilogue path are tested elsewhere; here use column sums directly
    xf = x.float()
    part = torch.stack([xf.sum(0), (xf * xf).sum(0)])[None].contiguous()
    rm, rv = rm0.clone(), rv0.clone()
    st = ops.bn_finalize(part, M, gamma, beta, rm, rv, 0.01, 1e-3, True)
    rm_ref, rv_ref = rm0.clone(), rv0.clone()
    xr = xf.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = F.batch_norm(xr, rm_ref, rv_ref, gr, br, True, 0.01, 1e-3)
    check(rm, rm_ref, 1e-4, "running mean")
    check(rv, rv_ref, 1e-4, "running var")
    check(st.scale * xf + st.shift, z.detach(), 1e-4, "bn affine")
    # forward apply with SiLU + rowscale + residual
    rs = torch.tensor([1.25, 0.0, 1.25, 1.25][:n_img], device=DEV)
    res = rnd(M, c, seed=36)
    out = ops.bnact_apply(x, n_img, hw, c, st.scale, st.shift, 1, rowscale=rs, res=res)
    ref = (F.silu(z.detach()).view(n_img, hw, c) * rs[:, None, None]).view(M, c) + res.float()
    check(out, ref, 1e-2, "bnact apply")
    pooled = ops.bnact_pool(x, n_img, hw, c, st.scale, st.shift, 1)
    check(pooled, F.silu(z.detach()).view(n_img, hw, c).mean(1), 1e-4, "bnact pool")
    # backward: y = silu(z) ; upstream = g*mul + add
    g = rnd(M, c, seed=37)
    mul = torch.sigmoid(rnd(n_img, c, seed=38, dtype=torch.float32))
    add = rnd(n_img, c, seed=39, dtype=torch.float32) * 0.01
    up = (g.float().view(n_img, hw, c) * mul[:, None, :] + add[:, None, :]).view(M, c)
    F.silu(z).backward(up)
    dx, dgamma, dbeta = ops.bnact_bwd(x, n_img, hw, c, st, gamma, 1, g=g, mul=mul, add=add)
    check(dx, xr.grad, 1.5e-2, "bn bwd dx")
    check(dgamma, gr.grad, 2e-3, "bn bwd dgamma")
    check(dbeta, br.grad, 2e-3, "bn bwd dbeta")
    dgate = ops.bnact_se_dgate(x, g, n_img, hw, c, st.scale, st.shift, 1)
    check(dgate, (g.float() * F.silu(z.detach())).view(n_img, hw, c).sum(1), 1e-4, "se dgate")
    # fused SE sums: same dgate, and BN-backward partials without a second pass
    sums = ops.bnact_se_sums(x, g, n_img, hw, c, st, 1)
    check(sums[0], dgate, 1e-5, "se sums dgate")
    part = ops.bn_partials_from_se_sums(sums, mul, add, 1.0)
    dx2, dgamma2, dbeta2 = ops.bnact_bwd(x, n_img, hw, c, st, gamma, 1, g=g, mul=mul, add=add, partials=part)
    check(dgamma2, gr.grad, 2e-3, "bn bwd dgamma (from se sums)")
    check(dbeta2, br.grad, 2e-3, "bn bwd dbeta (from se sums)")
    check(dx2, xr.grad, 1.5e-2, "bn bwd dx (from se sums)")


def test_bn_bwd_plain_rowscale_and_broadcast():
    n_img, hw, c = 3, 77, 40
    M = n_img * hw
    x = rnd(M, c, seed=40)
    gamma, beta = rnd(c, seed=41, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=42, dtype=torch.float32) * 0.2
    xf = x.float()
    part = torch.stack([xf.sum(0), (xf * xf).sum(0)])[None].contiguous()
    st = ops.bn_finalize(part, M, gamma, beta, None, None, 0.01, 1e-3, False)
    xr, gr, br = xf.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = F.batch_norm(xr, None, None, gr, br, True, 0.01, 1e-3)
    rs = torch.tensor([1.25, 0.0, 1.25], device=DEV)
    g = rnd(M, c, seed=43)
    (z.view(n_img, hw, c) * rs[:, None, None]).backward(g.float().view(n_img, hw, c))
    dx, dgamma, dbeta = ops.bnact_bwd(x, n_img, hw, c, st, gamma, 0, g=g, rowscale=rs)
    check(dx, xr.grad, 1.5e-2, "bn2 bwd dx")
    check(dgamma, gr.grad, 2e-3, "bn2 dgamma")
    check(dbeta, br.grad, 2e-3, "bn2 dbeta")
    # head: pooled-mean broadcast gradient
    xr.grad = None; gr.grad = None; br.grad = None
    z = F.batch_norm(xr, None, None, gr, br, True, 0.01, 1e-3)
    dpool = rnd(n_img, c, seed=44, dtype=torch.float32)
    F.silu(z).view(n_img, hw, c).mean(1).backward(dpool)
    dx, dgamma, dbeta = ops.bnact_bwd(x, n_img, hw, c, st, gamma, 1, add=dpool / hw)
    check(dx, xr.grad, 1.5e-2, "head bwd dx")
    check(dgamma, gr.grad, 2e-3, "head dgamma")


def test_bn_eval_coeffs():
    c = 48
    gamma, beta = rnd(c, seed=45, dtype=torch.float32), rnd(c, seed=46, dtype=torch.float32)
    rm, rv = rnd(c, seed=47, dtype=torch.float32), torch.rand(c, device=DEV) + 0.5
    st = ops.bn_eval_coeffs(gamma, beta, rm, rv, 1e-3)
    x = rnd(10, c, seed=48, dtype=torch.float32)
    check(x * st.scale + st.shift, F.batch_norm(x, rm, rv, gamma, beta, False, 0.0, 1e-3), 1e-5, "eval coeffs")


@pytest.mark.parametrize("n,c,cs", [(3, 48, 12), (2, 3072, 128), (5, 144, 6)])
def test_se_fwd_bwd(n, c, cs):
    pooled = rnd(n, c, seed=49, dtype=torch.float32).requires_grad_(True)
    w1 = (rnd(cs, c, seed=50, dtype=torch.float32) * c ** -0.5).requires_grad_(True)
    b1 = (rnd(cs, seed=51, dtype=torch.float32) * 0.1).requires_grad_(True)
    w2 = (rnd(c, cs, seed=52, dtype=torch.float32) * cs ** -0.5).requires_grad_(True)
    b2 = (rnd(c, seed=53, dtype=torch.float32) * 0.1).requires_grad_(True)
    gate_ref = torch.sigmoid(F.linear(F.silu(F.linear(pooled, w1, b1)), w2, b2))
    gate = ops.se_fwd(pooled.detach(), w1.detach(), b1.detach(), w2.detach(), b2.detach())
    check(gate, gate_ref.detach(), 1e-5, "se gate")
    dgate = rnd(n, c, seed=54, dtype=torch.float32)
    gate_ref.backward(dgate)
    dp, dw1, db1, dw2, db2 = ops.se_bwd(pooled.detach(), gate, dgate, w1.detach(), b1.detach(), w2.detach(), b2.detach())
    for got, ref, nm in [(dp, pooled.grad, "dpooled"), (dw1, w1.grad, "dw1"), (db1, b1.grad, "db1"),
                         (dw2, w2.grad, "dw2"), (db2, b2.grad, "db2")]:
        check(got, ref, 1e-4, "se " + nm)


def test_misc_cast_transpose_colsum_dropout():
    x = rnd(1000, 7, seed=55, dtype=torch.float32)
    assert torch.equal(ops.cast_bf16(x), x.to(BF))
    assert torch.equal(ops.cast_f32(x.to(BF)), x.to(BF).float())
    assert torch.equal(ops.transpose_f32(x), x.t().contiguous())
    m = rnd(5000, 240, seed=56)
    check(ops.colsum(m), m.float().sum(0), 1e-4, "colsum")
    m2 = rnd(33, 3072, seed=57)
    check(ops.colsum(m2), m2.float().sum(0), 1e-4, "colsum wide")
    v = torch.ones(200000, device=DEV)
    d1, d2 = ops.dropout_f32(v, 0.4, 1234, 7), ops.dropout_f32(v, 0.4, 1234, 7)
    assert torch.equal(d1, d2)
    keep = float((d1 > 0).float().mean())
    assert abs(keep - 0.6) < 0.01, keep
    assert abs(float(d1.max()) - 1 / 0.6) < 1e-5
    assert not torch.equal(d1, ops.dropout_f32(v, 0.4, 1234, 8))


# ------------------------------------------------------------------------------------------------ BERT pieces
@pytest.mark.parametrize("h", [64, 520])       # 520: 65 vectors, one lane in the second vector of the row
def test_bert_embed_fwd_bwd(h):
    b, t, vocab = 3, 16, 50
    g = torch.Generator().manual_seed(58)
    ids = torch.randint(0, vocab, (b, t), generator=g).to(DEV)
    tt = torch.zeros_like(ids)
    tt[0, 5:] = 1
    word = rnd(vocab, h, seed=59, dtype=torch.float32).requires_grad_(True)
    pos = rnd(32, h, seed=60, dtype=torch.float32).requires_grad_(True)
    typ = rnd(2, h, seed=61, dtype=torch.float32).requires_grad_(True)
    gamma = (rnd(h, seed=62, dtype=torch.float32) * 0.1 + 1).requires_grad_(True)
    beta = (rnd(h, seed=63, dtype=torch.float32) * 0.1).requires_grad_(True)
    ref = F.layer_norm(word[ids] + pos[torch.arange(t, device=DEV)][None] + typ[tt], (h,), gamma, beta, 1e-12)
    y, mean, rstd = ops.bert_embed_fwd(ids, tt, word.detach(), pos.detach(), typ.detach(), gamma.detach(), beta.detach(),
                                       1e-12, 0.0, 1, 0)
    check(y.view(b, t, h), ref.detach(), 1e-2, "embed fwd")
    dy = rnd(b * t, h, seed=64)
    ref.backward(dy.float().view(b, t, h))
    dword, dpos, dtyp, dgamma, dbeta = ops.bert_embed_bwd(dy, ids, tt, word.detach(), pos.detach(), typ.detach(),
                                                          gamma.detach(), mean, rstd, 0.0, 1, 0)
    for got, refg, nm in [(dword, word.grad, "dword"), (dpos, pos.grad, "dpos"), (dtyp, typ.grad, "dtype"),
                          (dgamma, gamma.grad, "dgamma"), (dbeta, beta.grad, "dbeta")]:
        check(got, refg, 2e-3, "embed " + nm)


@pytest.mark.parametrize("rows,h", [(37, 64), (300, 768),
                                    # vectors of 8 per lane: one vector in all, 63, exactly 64 (every lane once), 65, the limit 128
                                    (37, 8), (37, 504), (37, 512), (37, 520), (37, 1024)])
def test_add_ln_fwd_bwd(rows, h):
    x, res = rnd(rows, h, seed=65), rnd(rows, h, seed=66)
    gamma = (rnd(h, seed=67, dtype=torch.float32) * 0.1 + 1).requires_grad_(True)
    beta = (rnd(h, seed=68, dtype=torch.float32) * 0.1).requires_grad_(True)
    xr, rr = x.float().requires_grad_(True), res.float().requires_grad_(True)
    ref = F.layer_norm(xr + rr, (h,), gamma, beta, 1e-12)
    y, mean, rstd = ops.add_ln_fwd(x, res, gamma.detach(), beta.detach(), 1e-12, 0.0, 1, 0)
    check(y, ref.detach(), 1e-2, "add_ln fwd")
    dy = rnd(rows, h, seed=69)
    ref.backward(dy.float())
    dx, dres, dgamma, dbeta = ops.add_ln_bwd(dy, x, res, gamma.detach(), mean, rstd, 0.0, 1, 0)
    check(dx, xr.grad, 1.5e-2, "add_ln dx")
    check(dres, rr.grad, 1.5e-2, "add_ln dres")
    check(dgamma, gamma.grad, 2e-3, "add_ln dgamma")
    check(dbeta, beta.grad, 2e-3, "add_ln dbeta")


def test_add_ln_dropout_consistency():
    rows, h, p = 64, 768, 0.1
    x, res = rnd(rows, h, seed=70), torch.zeros(rows, h, device=DEV, dtype=BF)
    gamma, beta = torch.ones(h, device=DEV), torch.zeros(h, device=DEV)
    y1, m1, r1 = ops.add_ln_fwd(x, res, gamma, beta, 1e-12, p, 99, 3)
    y2, _, _ = ops.add_ln_fwd(x, res, gamma, beta, 1e-12, p, 99, 3)
    assert torch.equal(y1, y2)
    # the mask used by backward equals the forward mask: d/dx of sum(dres) only flows through kept elements
    dy = rnd(rows, h, seed=71)
    dx, dres, _, _ = ops.add_ln_bwd(dy, x, res, gamma, m1, r1, p, 99, 3)
    big = dres.float().abs() > 1e-3
    sel = (dx.float().abs() > 0) & big
    frac = float(sel.float().sum() / big.float().sum())
    assert abs(frac - 0.9) < 0.02, frac
    ratio = dx.float()[sel] / dres.float()[sel]
    assert float((ratio - 1 / 0.9).abs().max()) < 2e-2


@pytest.mark.parametrize("rows,t", [(300, 256), (301, 64), (77, 16), (130, 512), (50, 40), (33, 100)])
def test_softmax_fwd_bwd(rows, t):
    """t = 256 / 64 / 16 / 512: 8 keys per lane (32 / 8 / 2 / 64 lanes per row); 40 and 100: one key per lane-slot"""
    s = rnd(rows, t, seed=72, dtype=torch.float32) * 3
    s[:, (t * 3) // 4:] = -3.0e38
    sr = s.clone().requires_grad_(True)
    ref = torch.softmax(sr, -1)
    probs, pd = ops.softmax_fwd(s, 0.0, 1, 0)
    assert pd.data_ptr() == probs.data_ptr()
    check(probs, ref.detach(), 1e-2, "softmax")
    dp = rnd(rows, t, seed=73, dtype=torch.float32)
    ref.backward(dp)
    ds = ops.softmax_bwd(ref.detach().to(BF), dp, 0.0, 1, 0, 0.125)
    refds = sr.grad * 0.125
    # reference computed from the bf16-rounded probabilities the kernel sees
    pb = ref.detach().to(BF).float()
    refds2 = pb * (dp - (pb * dp).sum(-1, keepdim=True)) * 0.125
    check(ds, refds2, 1e-2, "softmax bwd")
    assert relerr(ds, refds) < 5e-2
    if t % 8:
        return                                              # dropout draws are per 8-element group
    probs2, pd2 = ops.softmax_fwd(s, 0.1, 5, 2)
    live = probs2[:, :(t * 3) // 4].float() > 0
    nz = float((pd2[:, :(t * 3) // 4].float() > 0)[live].float().mean())
    assert abs(nz - 0.9) < 0.03, nz
    # the backward regenerates the SAME mask from (seed, stream id): d/ds of sum(dp * dropout(softmax(s)))
    keep = (pd2.float() > 0).float() / 0.9
    pb2 = probs2.float()
    refds3 = pb2 * (dp * keep - (pb2 * dp * keep).sum(-1, keepdim=True)) * 0.125
    ds3 = ops.softmax_bwd(probs2, dp, 0.1, 5, 2, 0.125)
    sel = pb2 > 1e-3                                        # where a dropped probability is distinguishable from 0
    assert float((ds3.float() - refds3)[sel].abs().max()) <= 2e-2 * float(refds3.abs().max()) + 1e-3


def test_gelu_mask_eos():
    x = rnd(100, 3072, seed=74)
    check(ops.gelu_fwd(x), F.gelu(x.float()), 1e-2, "gelu")
    xr = x.float().requires_grad_(True)
    dy = rnd(100, 3072, seed=75)
    F.gelu(xr).backward(dy.float())
    check(ops.gelu_bwd(dy, x), xr.grad, 1e-2, "gelu bwd")
    b, t, h = 4, 16, 64
    lens = torch.tensor([16, 3, 9, 1], device=DEV)
    mask = (torch.arange(t, device=DEV)[None] < lens[:, None]).long()
    mb = ops.mask_bias(mask)
    assert float(mb[0].abs().max()) == 0 and float(mb[1, 3]) < -1e38
    hid = rnd(b * t, h, seed=76)
    out = ops.eos_gather(hid, mask, b, t, h)
    ref = hid.view(b, t, h).float()[torch.arange(b, device=DEV), lens - 1]
    assert torch.equal(out, ref)
    dh = ops.eos_scatter(ref, mask, b, t, h).view(b, t, h).float()
    assert torch.equal(dh[torch.arange(b, device=DEV), lens - 1], ref.to(BF).float())
    assert float(dh.abs().sum()) == pytest.approx(float(ref.to(BF).float().abs().sum()), rel=1e-5)


# ------------------------------------------------------------------------------------------------ heads / loss
def test_sgemm_l2norm_ce():
    b, d, n = 12, 512, 48
    a, bm = rnd(b, d, seed=77, dtype=torch.float32), rnd(n, d, seed=78, dtype=torch.float32)
    c = torch.empty(b, n, device=DEV)
    ops.sgemm(a, d, 1, bm, 1, d, c, n, b, n, d, alpha=14.0)         # a @ bm.T * 14
    check(c, 14.0 * a @ bm.T, 1e-5, "sgemm nt")
    c2 = torch.ones(d, n, device=DEV)
    ops.sgemm(a, 1, d, c, n, 1, c2, n, d, n, b, alpha=1.0, beta=0.5)   # a.T @ c + 0.5
    check(c2, a.T @ c + 0.5, 1e-5, "sgemm tn + beta")
    bias = rnd(n, seed=79, dtype=torch.float32)
    c3 = torch.empty(b, n, device=DEV)
    ops.sgemm(a, d, 1, bm, 1, d, c3, n, b, n, d, bias=bias)
    check(c3, a @ bm.T + bias, 1e-5, "sgemm bias")
    ar = a.clone().requires_grad_(True)
    yref = ar / ar.norm(dim=1, keepdim=True)
    y, nrm = ops.l2norm_fwd(a)
    check(y, yref.detach(), 1e-5, "l2norm")
    dy = rnd(b, d, seed=80, dtype=torch.float32)
    yref.backward(dy)
    check(ops.l2norm_bwd(dy, y, nrm), ar.grad, 1e-4, "l2norm bwd")
    logits = (rnd(b, n, seed=81, dtype=torch.float32) * 3).requires_grad_(True)
    labels = torch.arange(b, device=DEV) + 24
    lref = 0.25 * F.cross_entropy(logits, labels)
    lref.backward()
    buf = logits.detach().clone()
    loss = torch.zeros(1, device=DEV)
    ops.ce_fwd_bwd(buf, 24, 0.25, loss)
    check(loss[0], lref.detach(), 1e-5, "ce loss")
    check(buf, logits.grad, 1e-4, "ce dlogits")


def test_adamw_multi_tensor_vs_torch():
    """row N2: mc_adamw_step against torch.optim.AdamW (the reference's optimizer, optimizer/__init__.py:28-29) over
    ragged sizes (sub-vector, chunk-straddling, multi-chunk, > one 40-tensor launch), misaligned gradients (flat
    bucket views), a changing lr, and a state_dict hand-over in both directions.  fp32; a few ulp from operation order."""
    from mammo_clip_amd.breastclip.optimizer import AdamW
    torch.manual_seed(3)
    sizes = [1, 3, 7, 48, 1023, 4096, 16384, 16385, 50001, 3 * 16384 + 5] + [17 + i for i in range(60)] + [(300, 768)]
    mine = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in sizes]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    kw = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    om, ot = AdamW(mine, **kw), torch.optim.AdamW(ref, foreach=False, **kw)
    flat = torch.zeros(sum(p.numel() for p in mine) + 1, device=DEV)

    def set_grads(step):
        g = torch.Generator(device=DEV).manual_seed(100 + step)
        off = 1                                                    # every view starts 4 bytes off a 16-byte boundary
        for a, b in zip(mine, ref):
            v = flat[off:off + a.numel()].view_as(a)
            v.copy_(torch.randn(a.shape, device=DEV, generator=g) * (10.0 ** (step % 3 - 1)))
            a.grad = v if step % 2 else v.clone()
            b.grad = v.clone()
            off += a.numel()

    big = mine[-1]
    img0 = ops.cast_bf16(big.view(300, 768))                        # a cached bf16 image of a parameter ...
    for step in range(6):
        set_grads(step)
        for o in (om, ot):
            o.param_groups[0]["lr"] = 3e-3 * (0.5 + 0.1 * step)
        om.step(); ot.step()
        img = ops.cast_bf16(big.view(300, 768))                     # ... is rewritten by the optimizer kernel itself
        assert img is img0 and torch.equal(img, big.detach().to(BF).view(300, 768)), step
    om.state_dict()                                                  # step counters are materialised on demand
    for a, b in zip(mine, ref):
        torch.testing.assert_close(a, b, rtol=2e-6, atol=2e-7)
        torch.testing.assert_close(om.state[a]["exp_avg_sq"], ot.state[b]["exp_avg_sq"], rtol=2e-6, atol=1e-12)
        assert float(om.state[a]["step"]) == 6.0 and a._version >= 6     # in-place update is visible to autograd / caches
    # optimizer checkpoints move both ways [ref: trainer.py:215-237 saves optimizer.state_dict()]
    om2, ot2 = AdamW(mine, **kw), torch.optim.AdamW(ref, foreach=False, **kw)
    om2.load_state_dict(ot.state_dict()); ot2.load_state_dict(om.state_dict())
    set_grads(7)
    om2.step(); ot2.step()
    for a, b in zip(mine, ref):
        torch.testing.assert_close(a, b, rtol=2e-6, atol=4e-7)


# ---- the loss-scaled optimizer step (every step of the f16 storage build): mc_grads_unscale[_dev], mc_adamw_step_ls,
# mc_loss_scale_update and their host bookkeeping (AdamW.step_loss_scaled, engine.LossScaler) against torch.optim.AdamW +
# torch.amp.GradScaler.  All tensors fp32 on the device.  The common tensor set: sub-vector sizes, the last lane of the
# vector body (1023 / 1024), a ragged tail (1027), a chunk of 16384 exactly, a second chunk of length 1, three chunks, and
# 35 small tensors so that tensors 40 and up go into the second launch of a call (PACK = 40 in optim.hip).
LS_SIZES = [1, 3, 4, 5, 1023, 1024, 1027, 16384, 16385, 2 * 16384 + 3] + [17 + i for i in range(35)]
LS_LAYOUTS = ("own", "flat")
LS_HYPER = (3e-3, 0.9, 0.999, 1e-8, 0.05)                  # lr, beta1, beta2, eps, weight_decay
INF, NAN = float("inf"), float("nan")
FLT_MAX = torch.finfo(torch.float32).max


def _ls_normals(seed, scale=1.0, shapes=LS_SIZES):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(s if isinstance(s, tuple) else (s,), generator=g) * scale for s in shapes]


def _ls_place(host, layout):
    """device copies of the host tensors: "own" = one allocation each (16-byte aligned: the kernels' vector path), "flat" =
    views into one buffer that each start 4 bytes past a 16-byte boundary (scalar path)"""
    if layout == "own":
        out = [torch.empty_like(h, device=DEV).copy_(h) for h in host]
    else:
        offs, off = [], 1
        for h in host:
            offs.append(off)
            off += (h.numel() + 3) // 4 * 4                # the next view starts at 1 (mod 4) again
        flat = torch.zeros(off, device=DEV)
        out = [flat[o:o + h.numel()].view(h.shape) for o, h in zip(offs, host)]
        for o, h in zip(out, host):
            o.copy_(h)
    assert all((t.data_ptr() % 16 == 0) == (layout == "own") for t in out if t.numel())
    return out


def _ls_cat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _ls_table(grad, param=None, exp_avg=None, exp_avg_sq=None, image=None):
    """the mc_adamw_tensor table of a call, built like LossScaler._grad_table / AdamW._plan build theirs"""
    arr = (L.AdamwTensor * max(len(grad), 1))()
    for i, g in enumerate(grad):
        a = arr[i]
        a.grad, a.numel = g.data_ptr(), g.numel()
        if param is not None:
            a.param, a.exp_avg, a.exp_avg_sq = param[i].data_ptr(), exp_avg[i].data_ptr(), exp_avg_sq[i].data_ptr()
        if image is not None and image[i] is not None:
            a.bf16_image = image[i].data_ptr()
    return arr


def _ls_unscale(entry, arr, n, scale, flag):
    if entry == "mc_grads_unscale":                        # the host hands over 1 / scale, rounded once to fp32
        L.call(entry, arr, n, 1.0 / scale, flag.data_ptr(), ops._st())
    else:                                                  # the kernel divides by the device scale itself
        sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
        L.call(entry, arr, n, sc.data_ptr(), flag.data_ptr(), ops._st())
        torch.cuda.synchronize()                           # (sc is read through a raw pointer)


LS_UNSCALE_ENTRIES = ("mc_grads_unscale", "mc_grads_unscale_dev")


@pytest.mark.parametrize("entry", LS_UNSCALE_ENTRIES)
@pytest.mark.parametrize("layout", LS_LAYOUTS)
def test_grads_unscale_values(layout, entry):
    """grad *= 1 / scale over the common tensor set, gradients = seeded normals * 10^k.  A power-of-two scale (2^16, 2^-3)
    makes 1 / scale and the product exact: BIT-equal to torch's fp32 g * (1 / scale).  Scale 3000: within 4 fp32 ulp of the
    fp64 quotient, rtol 4 * 2^-23 = 4.8e-7 -- derived, not measured: one rounding in the reciprocal (1/2 ulp, on the host
    for mc_grads_unscale, a correctly rounded or at worst 2.5-ulp device division for mc_grads_unscale_dev), one in the
    product (1/2 ulp), the rest is headroom for the compiler's default fp32 division.  Zero-element tensors in the table
    (first, across the 40-tensor launch boundary, last) are skipped; n_tensors = 0 is a no-op that returns OK."""
    flag = torch.zeros(1, device=DEV)
    hole = torch.empty(0)
    for k in (-3, 0, 3):
        host = _ls_normals(40 + k, 10.0 ** k)
        host = [hole] + host[:39] + [hole] + host[39:] + [hole]
        src = _ls_cat(host).to(DEV)
        for scale in (2.0 ** 16, 2.0 ** -3, 3000.0):
            g = _ls_place(host, layout)
            _ls_unscale(entry, _ls_table(g), len(g), scale, flag)
            got = _ls_cat(g)
            if scale == 3000.0:
                torch.testing.assert_close(got.double(), src.double() / 3000.0, rtol=4.8e-7, atol=0.0)
            else:
                assert torch.equal(got, src * torch.tensor(1.0 / scale, dtype=torch.float32, device=DEV)), (k, scale)
            assert flag.item() == 0.0, (k, scale)
    g = _ls_place(_ls_normals(41), layout)
    want = _ls_cat(g).clone()
    _ls_unscale(entry, _ls_table(g), 0, 2.0, flag)                        # an empty call: nothing is touched
    if entry == "mc_grads_unscale":
        L.call(entry, None, 0, 0.5, flag.data_ptr(), ops._st())
    assert torch.equal(_ls_cat(g), want) and flag.item() == 0.0


# (tensor, element) of the one non-finite value: the 1-element tensor; the last lane of the vector body; the ragged tail
# after the last whole float4 (first and last element of it); a second chunk of length 1; the last element of the third
# chunk; the 45th tensor of the table, which the second launch of the call owns
LS_BAD_AT = [(0, 0), (5, 1023), (6, 1024), (6, 1026), (8, 16384), (9, 2 * 16384 + 2), (44, 10)]


@pytest.mark.parametrize("layout", LS_LAYOUTS)
def test_grads_unscale_flag(layout):
    """the non-finite flag against torch.isfinite: exactly 1.0 for one +inf / -inf / nan at every position of LS_BAD_AT (each
    value at each position, both entries, so every value meets the vector body, the ragged tail and the scalar path), every
    other element still unscaled BIT-exactly (scale 2^16); exactly 0.0 for finite gradients, +-FLT_MAX (scale 1) and fp32
    denormals included; a flag the caller left at 1 stays 1 (the launches of one call share it, the caller clears it)."""
    host = _ls_normals(50)
    g = _ls_place(host, layout)
    arr, n = _ls_table(g), len(g)
    clean = [t.clone() for t in g]
    starts = [0]
    for h in host:
        starts.append(starts[-1] + h.numel())
    flag = torch.zeros(1, device=DEV)
    scale = 2.0 ** 16
    ref = _ls_cat(clean) * torch.tensor(1.0 / scale, dtype=torch.float32, device=DEV)
    assert torch.isfinite(ref).all()
    for entry in LS_UNSCALE_ENTRIES:
        for ti, ei in LS_BAD_AT:
            assert ei < host[ti].numel()
            for bad in (INF, -INF, NAN):
                torch._foreach_copy_(g, clean)
                flag.zero_()
                g[ti][ei] = bad
                assert not torch.isfinite(_ls_cat(g)).all()
                _ls_unscale(entry, arr, n, scale, flag)
                got, at = _ls_cat(g), starts[ti] + ei
                assert flag.item() == 1.0, (entry, ti, ei, bad)
                v = got[at].item()
                assert v == bad or (bad != bad and v != v), (entry, ti, ei, bad, v)
                got[at] = ref[at]
                assert torch.equal(got, ref), (entry, ti, ei, bad)
    edge = {(0, 0): FLT_MAX, (5, 0): FLT_MAX, (5, 1023): -FLT_MAX, (6, 1024): FLT_MAX, (6, 1026): -FLT_MAX, (8, 16384): FLT_MAX,
            (9, 2 * 16384 + 2): -FLT_MAX, (44, 10): FLT_MAX, (7, 5): 1e-40, (6, 1025): -1e-40}
    for entry in LS_UNSCALE_ENTRIES:
        torch._foreach_copy_(g, clean)
        flag.zero_()
        for (ti, ei), val in edge.items():
            g[ti][ei] = val
        want = _ls_cat(g).clone()
        assert torch.isfinite(want).all() and (want.abs() == FLT_MAX).sum() == 8 and ((want != 0) & (want.abs() < 1e-38)).sum() == 2
        _ls_unscale(entry, arr, n, 1.0, flag)
        assert flag.item() == 0.0, entry                                  # torch.isfinite(want).all() says: clean
        assert torch.equal(_ls_cat(g), want), entry
        torch._foreach_copy_(g, clean)
        flag.fill_(1.0)
        _ls_unscale(entry, arr, n, scale, flag)
        assert flag.item() == 1.0 and torch.equal(_ls_cat(g), ref), entry


def _ls_adam_state(layout, seed):
    """param / grad / exp_avg / exp_avg_sq over a 2-D tensor, the common set and another 2-D tensor (47 tensors: 40 + 7),
    each 2-D parameter with a bf16 image.  exp_avg_sq >= max(exp_avg^2, grad^2), so that the updated moments keep
    |exp_avg| <= 1.0006 sqrt(exp_avg_sq) (Cauchy-Schwarz on 0.9 m + 0.1 g) like moments that come from real gradients."""
    shapes = [(43, 47)] + LS_SIZES + [(5, 7)]
    hp, hg, hm = _ls_normals(seed, 1.0, shapes), _ls_normals(seed + 1, 1.0, shapes), _ls_normals(seed + 2, 0.5, shapes)
    hv = [torch.maximum(m * m, g * g) * (1.0 + r.abs()) for m, g, r in zip(hm, hg, _ls_normals(seed + 3, 1.0, shapes))]
    host = (hp, hg, hm, hv)
    p, g, m, v = (_ls_place(h, layout) for h in host)
    image = [ops.cast_bf16(t) if t.dim() == 2 else None for t in p]
    return host, (p, g, m, v), image, _ls_table(g, p, m, v, image)


@pytest.mark.parametrize("layout", LS_LAYOUTS)
def test_adamw_step_ls_kernel(layout):
    """mc_adamw_step_ls.  Flag at 1: param, exp_avg, exp_avg_sq and the bf16 images are BIT-unchanged, for the tensors of both
    launches.  Flag at 0, host step t, device counter s: compared with mc_adamw_step(step = max(t - s, 1)) on a copy of the
    same state -- exp_avg / exp_avg_sq bit-equal (they do not depend on the bias scalars), param within one fp32 ulp, rtol
    2^-23 and atol 2^-22 * lr.  Derived: the two kernels run the same instructions and differ only in the last bit of
    step_size and 1 / sqrt(bias2), formed in double on the device instead of on the host (pow is not correctly rounded on
    either).  That moves the update u = step_size * m / denom by <= 2 * 2^-23 |u| plus three roundings of 2^-24 |u|, and
    |u| <= 0.32 * lr here (sqrt(bias2) / bias1 <= 0.316 for every applied step count, |m| <= 1.0006 sqrt(v)): < 2^-22 * lr;
    the final rounding of param - u adds one ulp of param, the rtol.  Bad arguments raise and launch nothing."""
    host, (p, g, m, v), image, arr = _ls_adam_state(layout, 60)
    n = len(p)
    flag, skipped = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    lr = LS_HYPER[0]

    def reset():
        for dst, src in zip((p, g, m, v), host):
            for d, s in zip(dst, src):
                d.copy_(s)

    def snap():
        return [_ls_cat(x).clone() for x in (p, m, v)] + [im.clone() for im in image if im is not None]

    before = snap()
    flag.fill_(1.0)
    L.call("mc_adamw_step_ls", arr, n, *LS_HYPER, 3, flag.data_ptr(), skipped.data_ptr(), ops._st())
    assert all(torch.equal(a, b) for a, b in zip(snap(), before)), "a flagged step wrote something"
    assert flag.item() == 1.0 and skipped.item() == 0.0
    for t, s in [(1, 0), (5, 0), (5, 2), (9, 8), (3, 3), (2, 5)]:
        reset()
        flag.zero_()
        skipped.fill_(float(s))
        L.call("mc_adamw_step_ls", arr, n, *LS_HYPER, t, flag.data_ptr(), skipped.data_ptr(), ops._st())
        got = snap()
        assert flag.item() == 0.0 and skipped.item() == float(s)         # the kernel only reads them
        for im, q in zip((im for im in image if im is not None), (q for q in p if q.dim() == 2)):
            assert torch.equal(im, q.to(BF)), (t, s)
        reset()
        L.call("mc_adamw_step", arr, n, *LS_HYPER, max(t - s, 1), ops._st())
        want = snap()
        assert not torch.equal(want[0], before[0])
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), (t, s)
        torch.testing.assert_close(got[0], want[0], rtol=2.0 ** -23, atol=2.0 ** -22 * lr, msg=lambda m_: f"(t, s) = {(t, s)}: {m_}")
    reset()
    torch.cuda.synchronize()
    before = snap()
    st = torch.tensor([1024.0, 1, 0, 2, 0, 0, 0, 0], dtype=torch.float32, device=DEV)
    for bad in [lambda: L.call("mc_adamw_step_ls", arr, n, *LS_HYPER, 2, None, skipped.data_ptr(), ops._st()),
                lambda: L.call("mc_adamw_step_ls", arr, n, *LS_HYPER, 2, flag.data_ptr(), None, ops._st()),
                lambda: L.call("mc_loss_scale_update", st.data_ptr(), skipped.data_ptr(), 2.0, 0.5, 0, 1, ops._st()),
                lambda: L.call("mc_loss_scale_update", st.data_ptr(), skipped.data_ptr(), 0.0, 0.5, 3, 1, ops._st()),
                lambda: L.call("mc_loss_scale_update", st.data_ptr(), skipped.data_ptr(), 2.0, -0.5, 3, 1, ops._st()),
                lambda: L.call("mc_loss_scale_update", None, skipped.data_ptr(), 2.0, 0.5, 3, 1, ops._st())]:
        with pytest.raises(L.MammoClipHipError):
            bad()
    assert all(torch.equal(a, b) for a, b in zip(snap(), before))
    assert st.tolist() == [1024.0, 1, 0, 2, 0, 0, 0, 0] and skipped.item() == 5.0


LS_FLAGS = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0]      # an overflow one step before growth, two in a row, two growths


def _gradscaler_trace(flags, init_scale, growth, backoff, interval):
    """(scale, clean steps in a row) after every update of a torch.amp.GradScaler on the device that sees ``flags``"""
    w = torch.nn.Parameter(torch.zeros(2, device=DEV))
    opt = torch.optim.AdamW([w], foreach=False)
    sc = torch.amp.GradScaler("cuda", init_scale=init_scale, growth_factor=growth, backoff_factor=backoff, growth_interval=interval)
    sc.scale(torch.zeros((), device=DEV))
    out = []
    for f in flags:
        w.grad = torch.full_like(w, INF if f else 0.0)
        sc.step(opt)
        sc.update()
        out.append((sc.get_scale(), int(sc.state_dict()["_growth_tracker"])))
    return out


def _policy_trace(flags, init_scale, growth, backoff, interval, dynamic=1, with_opt=True):
    """the 8 state floats (+ the optimizer's counter) after every mc_loss_scale_update that sees ``flags``"""
    st = torch.tensor([init_scale, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=DEV)
    osk = torch.zeros(1, device=DEV) if with_opt else None
    out = []
    for f in flags:
        st[2] = float(f)
        L.call("mc_loss_scale_update", st.data_ptr(), osk.data_ptr() if with_opt else None, growth, backoff, interval, dynamic,
               ops._st())
        out.append(st.tolist() + [osk.item() if with_opt else None])
    return out


@pytest.mark.parametrize("growth,backoff,with_opt", [(2.0, 0.5, True), (1.5, 0.3, True), (2.0, 0.5, False)])
def test_loss_scale_policy_vs_gradscaler(growth, backoff, with_opt):
    """mc_loss_scale_update against torch.amp.GradScaler("cuda", growth_interval=3) over LS_FLAGS: scale and clean-step
    counter BIT-equal after every update (torch multiplies the fp32 scale by its double factor and rounds once; so does the
    kernel), state[2] consumed, state[3] the running skip count, state[4] the outcome of the step, *opt_skipped follows."""
    ref = _gradscaler_trace(LS_FLAGS, 1024.0, growth, backoff, 3)
    assert len({s for s, _ in ref}) >= 3 and [t for _, t in ref].count(0) >= 5      # (the script moves the reference)
    got = _policy_trace(LS_FLAGS, 1024.0, growth, backoff, 3, with_opt=with_opt)
    for i, (row, (scale, tracker)) in enumerate(zip(got, ref)):
        nskip = float(sum(LS_FLAGS[:i + 1]))
        assert row[:5] == [scale, float(tracker), 0.0, nskip, float(LS_FLAGS[i])], (i, row, scale, tracker)
        assert row[5:8] == [0.0, 0.0, 0.0] and row[8] == (nskip if with_opt else None), (i, row)


def test_loss_scale_policy_static_and_range_bound():
    """dynamic = 0: scale and counter never move, skips are still counted and the flag is still consumed.  Range bound: from
    2^127 with growth_interval = 1 the scale stays 2^127 (GradScaler does not grow it to inf, after which every later step
    would be skipped) and the counter returns to 0, equal to torch."""
    for i, row in enumerate(_policy_trace(LS_FLAGS, 1024.0, 2.0, 0.5, 3, dynamic=0)):
        nskip = float(sum(LS_FLAGS[:i + 1]))
        assert row == [1024.0, 0.0, 0.0, nskip, float(LS_FLAGS[i]), 0.0, 0.0, 0.0, nskip], (i, row)
    ref = _gradscaler_trace([0, 0, 0], 2.0 ** 127, 2.0, 0.5, 1)
    got = _policy_trace([0, 0, 0], 2.0 ** 127, 2.0, 0.5, 1)
    print("range bound: torch", ref, "kernel", [r[:2] for r in got])
    for row, (scale, tracker) in zip(got, ref):
        assert math.isfinite(row[0]) and row[0] == 2.0 ** 127 and row[1] == 0.0, row
        assert row[:2] == [scale, float(tracker)], (row, scale, tracker)


def test_loss_scaled_steps_vs_torch_gradscaler():
    """The three launches and the host bookkeeping together: AdamW.step_loss_scaled + engine.LossScaler(1024, interval 4)
    against torch.optim.AdamW + torch.amp.GradScaler over 24 steps on the common tensor set plus a 2-D parameter with a
    cached bf16 image.  Both sides get the same scaled gradients (seeded normals * the reference scaler's scale, a changing
    lr); an inf lands in one gradient on steps 1 (early), 6 and 7 (in a row), 11 (the step that would have grown the scale),
    14, 17 and 22.  After every step: parameters at the plain kernel's tolerances (rtol 2e-6, atol 2e-7), scale and
    clean-step counter bit-equal to GradScaler's, the image bit-equal to param.to(BF).  After 12 steps state_dict() holds
    the APPLIED step count (8) on both sides and each optimizer continues from the other's state (load_state_dict and
    _sync_steps under a non-zero device counter); on steps 16 and 17 one parameter has no gradient (the plan is rebuilt
    while the device counter is non-zero: _fold_skipped; afterwards that parameter's count lags: the per-step-count launch
    loop with the loss-scale tail); two plain step() calls at the end fold the counter at the top of step(), the second of
    them again without that parameter's gradient: a plan rebuilt between plain steps must carry on from the counts of the
    plan it replaces, not from the step counts of the last state_dict() call."""
    from mammo_clip_amd import engine
    from mammo_clip_amd.breastclip.optimizer import AdamW
    shapes = LS_SIZES + [(43, 47)]
    mine = [torch.nn.Parameter(h.to(DEV)) for h in _ls_normals(70, 1.0, shapes)]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    kw = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    om, ot = AdamW(mine, **kw), torch.optim.AdamW(ref, foreach=False, **kw)
    sm = engine.LossScaler(init_scale=1024.0, growth_interval=4)
    st = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=4)
    st.scale(torch.zeros((), device=DEV))
    bad_at = {1: 4, 6: 0, 7: 9, 11: 44, 14: 6, 17: 8, 22: 45}             # step -> the tensor whose gradient gets the inf
    lagging, no_grad_steps = 7, (16, 17, 25)
    offs, off = [], 1
    for p in mine:
        offs.append(off)
        off += (p.numel() + 3) // 4 * 4
    flat = torch.zeros(off, device=DEV)
    big, img0 = mine[-1], ops.cast_bf16(mine[-1])
    need, applied, growths = [], 0, 0

    def set_grads(step, scale):
        gen = torch.Generator(device=DEV).manual_seed(200 + step)
        for i, (a, b) in enumerate(zip(mine, ref)):
            v = flat[offs[i]:offs[i] + a.numel()].view_as(a)              # 4 bytes off a 16-byte boundary
            v.copy_(torch.randn(a.shape, device=DEV, generator=gen) * (10.0 ** (step % 3 - 1) * scale))
            if bad_at.get(step) == i:
                v.view(-1)[v.numel() // 2] = INF
            a.grad = v if step % 2 else v.clone()
            b.grad = v.clone()
            if step in no_grad_steps and i == lagging:
                a.grad = b.grad = None

    def compare(step, atol=2e-7):
        a, b = _ls_cat([p.detach() for p in mine]), _ls_cat([p.detach() for p in ref])
        assert torch.isfinite(a).all(), step
        need.append(float(((a - b).abs() - 2e-6 * b.abs()).max()))     # the atol this step needs next to rtol 2e-6
        img = ops.cast_bf16(big)
        assert img is img0 and torch.equal(img, big.detach().to(BF)), step

    for step in range(24):
        if step == 12:
            sdm, sdt = om.state_dict(), ot.state_dict()
            assert int(om._ls_skipped.item()) == 4
            for i in range(len(mine)):
                assert float(sdm["state"][i]["step"]) == float(sdt["state"][i]["step"]) == 8.0, i
            om, ot = AdamW(mine, **kw), torch.optim.AdamW(ref, foreach=False, **kw)
            om.load_state_dict(sdt)
            ot.load_state_dict(sdm)
        scale, tracker = st.get_scale(), int(st.state_dict()["_growth_tracker"])
        if step == 11:
            assert tracker == 3                                           # a clean step 11 would have grown the scale
        set_grads(step, scale)
        for o in (om, ot):
            o.param_groups[0]["lr"] = 3e-3 * (0.5 + 0.1 * (step % 7))
        sm.unscale_(mine)
        sm.update(om.step_loss_scaled(sm))
        st.step(ot)
        st.update()
        applied += step not in bad_at
        growths += st.get_scale() > scale
        assert sm.scale == st.get_scale() and sm.state_dict()["growth_tracker"] == int(st.state_dict()["_growth_tracker"]), step
        assert sm.skipped == step + 1 - applied and sm.last_skipped == (step in bad_at), step
        compare(step)
        if step in (16, 18):                                              # a plan rebuilt under a non-zero device counter
            assert int(om._ls_skipped.item()) == 0
    assert applied == 17 and growths == 2
    sdm, sdt = om.state_dict(), ot.state_dict()
    for i in range(len(mine)):
        assert float(sdm["state"][i]["step"]) == float(sdt["state"][i]["step"]) == (16.0 if i == lagging else 17.0), i
    assert int(om._ls_skipped.item()) == 1                                # step 22, not folded yet
    for step in (24, 25):                             # plain steps on unscaled gradients; 25 rebuilds the plan once more
        set_grads(step, 1.0)
        om.step()
        ot.step()
        compare(step)
    print("atol needed next to rtol 2e-6, per step:", " ".join(f"{x:.1e}" for x in need))
    assert max(need) <= 2e-7, need
    sdm, sdt = om.state_dict(), ot.state_dict()
    for i, (a, b) in enumerate(zip(mine, ref)):
        torch.testing.assert_close(om.state[a]["exp_avg_sq"], ot.state[b]["exp_avg_sq"], rtol=2e-6, atol=1e-12)
        assert float(sdm["state"][i]["step"]) == float(sdt["state"][i]["step"]) == (17.0 if i == lagging else 19.0), i


def test_raw_u8_input_pipeline_matches_host_normalisation():
    """row N4: uint8 pixels + (mean, std) through the stem's fused load == the dataset's host-side normalisation
    [ref: imagetext.py:131-135] followed by the fp32 path, BIT for bit (same float32 operation order), for the
    trainer's permuted [b,1,H,W,3] view (trainer_ddp.py:288-291) and for a plain NCHW batch; forward and the stem's
    weight gradient.  Images with different ranges per sample, one of them with 3 distinct channels."""
    import numpy as np
    from oracle import inputs as oin
    from mammo_clip_amd.breastclip.model.modules import load_image_encoder
    rng = np.random.default_rng(5)
    b, H, W = 3, 70, 54
    mean, std = 0.3089279, 0.25053555408335154                      # pre_train_b5_clip.yaml:23-24
    raw = np.stack([np.repeat(rng.integers(lo, hi, size=(H, W, 1), dtype=np.uint8), 3, axis=2)
                    for lo, hi in ((0, 256), (17, 201), (90, 131))])
    raw[2] = rng.integers(3, 250, size=(H, W, 3), dtype=np.uint8)
    ref = np.stack([oin.normalize_u8(raw[i], mean, std) for i in range(b)])           # [b,H,W,3] float32
    enc = load_image_encoder({"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": False, "model_type": "cnn"}).to(DEV)
    enc.eval()
    x_f = torch.from_numpy(ref).to(DEV).unsqueeze(1).squeeze(1).permute(0, 3, 1, 2)    # trainer's view of [b,1,H,W,3]
    u8 = torch.from_numpy(raw).to(DEV)
    for x_u in (u8.unsqueeze(1).squeeze(1).permute(0, 3, 1, 2), u8.permute(0, 3, 1, 2).contiguous()):
        l, r, t, bb = enc.stem_pad
        oh, ow = (H + t + bb - 3) // 2 + 1, (W + l + r - 3) // 2 + 1
        pa = ops.stem_im2col(x_f, l, t, oh, ow)
        pb = ops.stem_im2col(ops.RawImages(x_u, mean, std), l, t, oh, ow)
        assert torch.equal(pa, pb)
        with torch.no_grad():
            ya, yb = enc(x_f), enc(ops.RawImages(x_u, mean, std))
        assert torch.equal(ya, yb)
    mm = ops.image_minmax_u8(u8)
    assert mm.tolist() == [[int(raw[i].min()) for i in range(b)], [int(raw[i].max()) for i in range(b)]]
    enc.train()
    ga = []
    for x in (x_f, ops.RawImages(u8.permute(0, 3, 1, 2), mean, std)):
        enc.zero_grad(set_to_none=True)
        enc.rng.seed, enc.rng.calls = 1234, 0
        enc(x).square().sum().backward()
        ga.append(enc._conv_stem.weight.grad.clone())
    assert torch.equal(ga[0], ga[1])


def test_raw_u8_input_pipeline_vs_reference_fixture():
    """row N4 pinned by the REFERENCE: tests/golden/input_pipeline.npz holds raw uint8 pixels and the float32 batch
    tensor the reference's ImageTextDataset.__getitem__ + collate_fn + trainer permute made of them [ref:
    imagetext.py:67-234, trainer_ddp.py:288-291].  The stem's fused uint8 load must see exactly those values: its patch
    matrix from the uint8 batch equals, bit for bit, the patch matrix built from the reference's float32 tensor."""
    import numpy as np
    import os
    from mammo_clip_amd.breastclip.model.modules import load_image_encoder
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "input_pipeline.npz"))
    mean, std = float(z["mean_std"][0]), float(z["mean_std"][1])
    enc = load_image_encoder({"source": "cnn", "name": "tf_efficientnet_b5_ns-detect", "pretrained": False, "model_type": "cnn"}).to(DEV)
    enc.eval()
    l, r, t, bb = enc.stem_pad
    for key in ("images", "image_views"):
        ref = torch.from_numpy(z["out/" + key]).to(DEV)                       # [b,3,H,W] float32, the model's input
        u8 = torch.from_numpy(z["raw/" + key]).to(DEV)                        # [b,H,W,3] uint8
        b, _, H, W = ref.shape
        oh, ow = (H + t + bb - 3) // 2 + 1, (W + l + r - 3) // 2 + 1
        pa = ops.stem_im2col(ref, l, t, oh, ow)
        pb = ops.stem_im2col(ops.RawImages(u8.unsqueeze(1).squeeze(1).permute(0, 3, 1, 2), mean, std), l, t, oh, ow)
        assert torch.equal(pa, pb), key
        with torch.no_grad():
            assert torch.equal(enc(ref), enc(ops.RawImages(u8.permute(0, 3, 1, 2), mean, std)))


def test_torch_library_custom_ops():
    """the ``mammoclip::`` operators (custom_ops.py) run the same kernels as the ops.py wrappers, are differentiable where
    an explicit backward op is registered, and pass torch.library.opcheck (schema, fake tensor, autograd registration)."""
    import mammo_clip_amd.custom_ops  # noqa: F401
    x = rnd(300, 64, seed=1).requires_grad_(True)
    w = rnd(48, 64, seed=2, scale=0.125).requires_grad_(True)
    b = rnd(48, seed=3, dtype=torch.float32)
    y = torch.ops.mammoclip.linear(x, w, b)
    assert torch.equal(y, ops.linear_fwd(x.detach(), w.detach(), bias=b))
    g = rnd(300, 48, seed=4)
    y.backward(g)
    check(x.grad, g.float() @ w.detach().float(), 1e-2, "custom op dx")
    check(w.grad, g.float().T @ x.detach().float(), 1e-2, "custom op dw")
    n, h, wd, c, k = 2, 9, 7, 16, 3
    xi = rnd(n * h * wd, c, seed=5).requires_grad_(True)
    wk = rnd(k * k, c, seed=6, dtype=torch.float32)
    yo = torch.ops.mammoclip.dwconv(xi, wk, n, h, wd, k, 1, 1, 1, h, wd)
    ref = F.conv2d(xi.detach().float().view(n, h, wd, c).permute(0, 3, 1, 2), wk.T.reshape(c, 1, k, k), padding=1, groups=c)
    check(yo, ref.permute(0, 2, 3, 1).reshape(n * h * wd, c), 1e-2, "custom op dwconv")
    yo.backward(rnd(n * h * wd, c, seed=7))
    assert xi.grad is not None and torch.isfinite(xi.grad.float()).all()
    check(torch.ops.mammoclip.gelu(xi.detach()), F.gelu(xi.detach().float()), 1e-2, "custom op gelu")
    torch.library.opcheck(torch.ops.mammoclip.linear.default, (x.detach(), w.detach(), b), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.mammoclip.gelu.default, (xi.detach(),), test_utils=("test_schema", "test_faketensor"))


def _e4m3(x, amax):
    """torch reference of the per-tensor e4m3 quantisation: dequantised values and the scale"""
    scale = 448.0 / amax
    q = (x.float() * scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.float() / scale


@pytest.mark.parametrize("M,N,K", [(3000, 1824, 304), (4096, 512, 3072), (700, 304, 1824), (256, 2048, 512), (5000, 96, 48)])
def test_fp8_quant_and_gemm(M, N, K):
    """config #5 building blocks: (1) the quantisation kernel reproduces torch's float8_e4m3fn conversion (OCP e4m3, the
    format gfx950's fp8 MFMA reads) byte for byte; (2) the fp8 GEMM equals the fp32 product of the DEQUANTISED operands
    up to the bf16 rounding of its output (<= 1e-2 of max|ref|): every fp8 x fp8 product is exact in fp32."""
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    ax, aw = ops.amax_bf16(x), ops.amax_bf16(w)
    assert float(ax) == float(x.float().abs().max()) and float(aw) == float(w.float().abs().max())
    xq, sx = ops.quant_fp8(x, ax)
    refq = (x.float() * (448.0 / float(ax))).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    assert torch.equal(xq.view(torch.uint8), refq.view(torch.uint8))
    assert abs(float(sx) - float(ax) / 448.0) <= 1e-9 * float(ax)
    y, part = ops.linear_fwd_fp8(x, w, stats=True)
    ref = _e4m3(x, float(ax)) @ _e4m3(w, float(aw)).T
    check(y, ref, 1e-2, "fp8 gemm vs dequantised fp32 product")
    s = part.double().sum(0)
    check(s[0].float(), y.float().double().sum(0).float(), 1e-4, "fp8 gemm colsum")
    # and it stays close to the unquantised product (e4m3: 3 mantissa bits -> ~6 % per element, averaging out over K)
    full = x.float() @ w.float().T
    assert relerr(y, full) <= 0.08 * (1 + 64.0 / K) ** 0.5 + 0.02, relerr(y, full)


def test_fp8_batched_gated_weights():
    nb, hw, N, K = 5, 700, 304, 1824
    x, w = rnd(nb * hw, K, seed=7), rnd(N, K, seed=8, scale=K ** -0.5)
    gate = torch.sigmoid(rnd(nb, K, seed=9, dtype=torch.float32))
    wg = ops.gate_weights(w, gate)
    check(wg, (w.float()[None] * gate[:, None, :]), 1e-2, "gated weights")
    y = ops.linear_fwd_fp8(x, wg, batch_w=(nb, hw))
    ax, aw = float(x.float().abs().max()), float(wg.float().abs().max())
    ref = torch.einsum("bmk,bnk->bmn", _e4m3(x, ax).view(nb, hw, K), _e4m3(wg, aw)).reshape(nb * hw, N)
    check(y, ref, 1e-2, "fp8 batched gemm")


@pytest.mark.parametrize("k,n,h,w,c", [(3, 2, 40, 33, 240), (5, 2, 29, 23, 384), (3, 3, 17, 50, 144), (5, 1, 60, 64, 64), (3, 2, 20, 20, 24)])
def test_dwconv_dgrad_with_bn_backward_epilogue(k, n, h, w, c):
    """stride-1 depthwise data gradient with the fused BatchNorm(+SiLU)-backward epilogue (mc_dwconv_args.epi_x) ==
    plain data gradient followed by the two-pass BatchNorm backward: dE, dgamma, dbeta (bf16 round-off: the fused path
    rounds dZ once more, <= 1.5e-2 of max|ref|)."""
    pad = (k - 1) // 2
    e = rnd(n * h * w, c, seed=1)
    dd = rnd(n * h * w, c, seed=2)
    wk = rnd(k * k, c, seed=3, dtype=torch.float32)
    gamma, beta = rnd(c, seed=4, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=5, dtype=torch.float32) * 0.1
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(n * h * w)
    wflip = wk.flip(0).contiguous()
    da0 = ops.dwconv_bwd_data(dd, wk, n, h, w, c, k, 1, pad, pad, h, w, w_kkc_flipped=wflip)
    de_ref, dg_ref, db_ref = ops.bnact_bwd(e, n, h * w, c, st, gamma, 1, g=da0)
    dz, part = ops.dwconv_bwd_data(dd, wk, n, h, w, c, k, 1, pad, pad, h, w, w_kkc_flipped=wflip, epi=(e, st))
    de, dg, db = ops.bnact_bwd(e, n, h * w, c, st, gamma, 0, g=dz, partials=part)
    z = ef * st.scale + st.shift
    sg = torch.sigmoid(z)
    check(dz, da0.float() * (sg * (1 + z * (1 - sg))), 1.5e-2, "dZ0")
    check(de, de_ref, 1.5e-2, "dE through the fused epilogue")
    check(dg, dg_ref, 1e-2, "dgamma")
    check(db, db_ref, 1e-2, "dbeta")


LANE_CASES = [  # k, s, n, h, w, c: several strips per row (w > 124 / 62), several items per workgroup, ragged channel tiles
    (5, 1, 3, 150, 260, 96), (5, 1, 5, 95, 57, 72), (5, 1, 2, 61, 130, 40), (3, 1, 2, 70, 300, 48), (3, 1, 3, 33, 59, 24),
    (5, 2, 2, 120, 250, 48), (3, 2, 3, 77, 131, 40), (5, 1, 33, 48, 29, 32), (5, 1, 1, 300, 114, 64),
    (5, 1, 70, 1100, 40, 32),    # > 128 blocks per workgroup: the descriptor ring is refilled (twice)
    (5, 1, 5, 6, 5, 40), (3, 1, 9, 7, 9, 24), (5, 2, 3, 9, 11, 16)]   # tiny maps, image groups with a ragged last group


@pytest.mark.parametrize("k,s,n,h,w,c", LANE_CASES)
@pytest.mark.parametrize("use_pro", [False, True])
def test_dwconv_lane_form_equals_marching_form(k, s, n, h, w, c, use_pro):
    """Round 4: the lane = column depthwise kernels (conv_lane.hip) against the marching kernels on the same inputs -- both
    add an output's taps in the same order with fp32 FMAs, so the OUTPUT is bit-identical; the BatchNorm statistics
    partials are sums of the same stored values in a different order (<= 2e-5 of the largest column sum)."""
    Lh = L.load()
    pad = (k - 1) // 2 if s == 1 else (k - 2) // 2
    oh, ow = (h + s - 1) // s, (w + s - 1) // s
    x = rnd(n * h * w, c, seed=31)
    wk = rnd(k * k, c, seed=32, dtype=torch.float32) * 0.3
    pro = (rnd(c, seed=33, dtype=torch.float32) * 0.3 + 1.0, rnd(c, seed=34, dtype=torch.float32) * 0.3) if use_pro else None
    out = {}
    old = Lh.mc_dwconv_set_lane_mode(0)
    try:
        for mode in (0, 1):
            Lh.mc_dwconv_set_lane_mode(mode)
            out[mode] = ops.dwconv_fwd(x, wk, n, h, w, c, k, s, pad, pad, oh, ow, pro=pro, stats=True)
    finally:
        Lh.mc_dwconv_set_lane_mode(old)
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]), "lane-form output differs from the marching form"
    s0, s1 = out[0][1].double().sum(0), out[1][1].double().sum(0)
    assert float((s0 - s1).abs().max()) <= 2e-5 * float(s0.abs().max()), "statistics partials"


@pytest.mark.parametrize("k,s,n,h,w,c", LANE_CASES)
def test_dwconv_lane_weight_gradient_equals_marching_form(k, s, n, h, w, c):
    """the weight-gradient mode of the lane = column kernel against the marching weight-gradient kernel (both sum fp32
    products of the same bf16 operands, in different orders: <= 2e-4 of the largest tap gradient; run twice -- the second
    launch finds whatever the first left in LDS)"""
    Lh = L.load()
    pad = (k - 1) // 2 if s == 1 else (k - 2) // 2
    oh, ow = (h + s - 1) // s, (w + s - 1) // s
    x = rnd(n * h * w, c, seed=41)
    dy = rnd(n * oh * ow, c, seed=42)
    pro = (rnd(c, seed=33, dtype=torch.float32) * 0.3 + 1.0, rnd(c, seed=34, dtype=torch.float32) * 0.3)
    out = {}
    old = Lh.mc_dwconv_set_lane_mode(0)
    try:
        for mode in (0, 1, 1):
            Lh.mc_dwconv_set_lane_mode(mode)
            out[mode] = ops.dwconv_bwd_weight(x, dy, n, h, w, c, k, s, pad, pad, oh, ow, pro=pro)
    finally:
        Lh.mc_dwconv_set_lane_mode(old)
    assert torch.isfinite(out[1]).all()
    assert float((out[0] - out[1]).abs().max()) <= 2e-4 * float(out[0].abs().max())


@pytest.mark.parametrize("k,n,h,w,c", [(5, 3, 150, 260, 96), (5, 5, 95, 57, 72), (3, 2, 70, 300, 48), (5, 33, 48, 29, 32)])
def test_dwconv_lane_form_epilogue_equals_marching_form(k, n, h, w, c):
    """the same for the stride-1 data gradient with the BatchNorm-backward epilogue (dZ0 bit-identical, partials to 2e-5)"""
    Lh = L.load()
    pad = (k - 1) // 2
    e = rnd(n * h * w, c, seed=1)
    dd = rnd(n * h * w, c, seed=2)
    wk = rnd(k * k, c, seed=3, dtype=torch.float32)
    gamma, beta = rnd(c, seed=4, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=5, dtype=torch.float32) * 0.1
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(n * h * w)
    wflip = wk.flip(0).contiguous()
    out = {}
    old = Lh.mc_dwconv_set_lane_mode(0)
    try:
        for mode in (0, 1):
            Lh.mc_dwconv_set_lane_mode(mode)
            out[mode] = ops.dwconv_bwd_data(dd, wk, n, h, w, c, k, 1, pad, pad, h, w, w_kkc_flipped=wflip, epi=(e, st))
    finally:
        Lh.mc_dwconv_set_lane_mode(old)
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]), "lane-form dZ0 differs from the marching form"
    s0, s1 = out[0][1].double().sum(0), out[1][1].double().sum(0)
    scale = s0.abs().amax(dim=1, keepdim=True)
    assert float(((s0 - s1).abs() / scale).max()) <= 2e-4, "BatchNorm-backward partials"


@pytest.mark.parametrize("M,N,K", [(9000, 144, 24), (20000, 240, 40), (8200, 384, 64), (8192, 96, 16), (12345, 288, 48), (70001, 240, 40)])
@pytest.mark.parametrize("with_res", [False, True])
def test_xbwd_rows_both_gradients_from_one_pass(M, N, K, with_res):
    """Round 5: mc_xbwd_rows_bf16 -- weight gradient dW = dY^T x AND data gradient dX = dY . Wt^T (+ R) of a 1x1 convolution
    from one pass over dY [ref: backward of efficientnet_custom.py:104] -- against the two launches it replaces (the same MFMA
    products in the same per-row order: dX identical to mc_gemm_rows_bf16 up to one 16-bit ulp of the rounding of the sum with
    the residual; dW to the fp32 summation order) and against fp32 torch.  Ragged row counts: the last step is partial."""
    assert ops.xbwd_rows_ok(M, N, K)
    dy, x = rnd(M, N, seed=1), rnd(M, K, seed=2)
    w = rnd(N, K, seed=3, scale=K ** -0.5)                     # W [N, K]; the data gradient's operand is W^T
    w_t = w.t().contiguous()
    res = rnd(M, K, seed=4) if with_res else None
    dx_sep = ops.linear_dgrad(dy, w, residual=res, w_t=w_t)
    dw_sep = ops.linear_wgrad(dy, x)
    for _ in range(2):
        dx, dw = ops.xbwd_rows(dy, x, w_t, residual=res)
    torch.cuda.synchronize()
    ref_dx = dy.float() @ w.float() + (res.float() if with_res else 0.0)
    check(dx, ref_dx, 1e-2, "dX vs fp32")
    check(dx, dx_sep.float(), 8e-3, "dX vs the row-streaming data gradient")
    ref_dw = dy.float().t() @ x.float()
    check(dw, ref_dw, 2e-3, "dW vs fp32")
    assert float((dw - dw_sep).abs().max()) <= 2e-4 * float(dw_sep.abs().max()), "dW vs the row-streaming weight gradient"


FUSED_CASES = [  # n, h, w, c: several strips per row (w > 62), image groups (w <= 30 / 14), ragged channel tiles, tiny maps
    (2, 70, 300, 48), (3, 33, 59, 24), (5, 95, 57, 72), (33, 48, 29, 64), (9, 7, 9, 24), (2, 40, 33, 240), (1, 200, 62, 40),
    (70, 600, 40, 32)]   # > 128 blocks per workgroup: the descriptor ring is refilled


@pytest.mark.parametrize("n,h,w,c", FUSED_CASES)
def test_dwconv_fused_backward_equals_the_two_launches(n, h, w, c):
    """Round 5: the whole stride-1 3x3 depthwise backward in ONE launch (conv_lane.hip MODE 3, ops.dwconv_bwd_fused) against the
    two launches it replaces on the same inputs [ref: efficientnet_custom.py:104-111 backwards]:
      * dZ0 and the BatchNorm0-backward partials: the data-gradient launch with the epilogue (the fused kernel adds the taps of
        an output in the same order: dZ0 bit-identical; partials to 2e-4 of the column's scale),
      * dW: the weight-gradient launch with the BN0 + SiLU prologue (the separate launch rounds the activated input to the
        16-bit storage type while staging, the fused launch keeps fp32: <= 4e-3 of the largest tap gradient) and an fp32 torch
        reference of dW[t, c] = sum dd[o] * silu(bn0(e))[o + t - pad] (<= 4e-3: 16-bit dd, fp32 sums).
    Run twice: the second launch finds whatever the first left in LDS."""
    k, pad = 3, 1
    e = rnd(n * h * w, c, seed=1)
    dd = rnd(n * h * w, c, seed=2)
    wk = rnd(k * k, c, seed=3, dtype=torch.float32)
    gamma, beta = rnd(c, seed=4, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=5, dtype=torch.float32) * 0.1
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(n * h * w)
    wflip = wk.flip(0).contiguous()
    assert ops.dwconv_bwd_fused_ok(n, h, w, c, k, 1, pad, pad, h, w, force=True)
    dz_ref, part_ref = ops.dwconv_bwd_data(dd, wk, n, h, w, c, k, 1, pad, pad, h, w, w_kkc_flipped=wflip, epi=(e, st))
    dw_sep = ops.dwconv_bwd_weight(e, dd, n, h, w, c, k, 1, pad, pad, h, w, pro=(st.scale, st.shift))
    for _ in range(2):
        dz, part, dw = ops.dwconv_bwd_fused(dd, e, st, wflip, n, h, w, c, k, pad, pad, h, w)
    torch.cuda.synchronize()
    assert torch.equal(dz, dz_ref), "fused dZ0 differs from the data-gradient launch"
    s0, s1 = part_ref.double().sum(0), part.double().sum(0)
    scale = s0.abs().amax(dim=1, keepdim=True)
    assert float(((s0 - s1).abs() / scale).max()) <= 2e-4, "BatchNorm-backward partials"
    assert torch.isfinite(dw).all()
    assert float((dw - dw_sep).abs().max()) <= 4e-3 * float(dw_sep.abs().max()), "dW vs the separate weight-gradient launch"
    a0 = torch.nn.functional.silu(ef * st.scale + st.shift).view(n, h, w, c).permute(0, 3, 1, 2)
    a0p = torch.nn.functional.pad(a0, (pad, pad, pad, pad))
    g = dd.float().view(n, h, w, c).permute(0, 3, 1, 2)
    ref = torch.stack([(g * a0p[:, :, kh:kh + h, kw:kw + w]).sum((0, 2, 3)) for kh in range(k) for kw in range(k)])
    check(dw, ref, 4e-3, "dW vs fp32 reference")


@pytest.mark.parametrize("k,n,h,w,c,pad", [(3, 2, 40, 33, 144, (0, 1)), (3, 2, 41, 34, 240, (1, 1)), (5, 2, 29, 23, 384, (1, 2)),
                                          (5, 1, 60, 64, 64, (2, 2)), (3, 3, 17, 50, 48, (0, 0)), (5, 2, 30, 31, 1056, (2, 1))])
def test_dwconv_s2_dgrad_with_bn_backward_epilogue(k, n, h, w, c, pad):
    """stride-2 depthwise data gradient (marching super-pixel kernel) with the fused BatchNorm(+SiLU)-backward epilogue ==
    plain stride-2 data gradient followed by the two-pass BatchNorm backward (static "same" padding incl. the asymmetric
    forms, odd and even maps): dZ0, dE, dgamma, dbeta."""
    pl, pt = pad
    oh, ow = (h + 1) // 2, (w + 1) // 2
    e = rnd(n * h * w, c, seed=1)
    dd = rnd(n * oh * ow, c, seed=2)
    wk = rnd(k * k, c, seed=3, dtype=torch.float32)
    gamma, beta = rnd(c, seed=4, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=5, dtype=torch.float32) * 0.1
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(n * h * w)
    da0 = ops.dwconv_bwd_data(dd, wk, n, h, w, c, k, 2, pl, pt, oh, ow)
    de_ref, dg_ref, db_ref = ops.bnact_bwd(e, n, h * w, c, st, gamma, 1, g=da0)
    dz, part = ops.dwconv_bwd_data(dd, wk, n, h, w, c, k, 2, pl, pt, oh, ow, epi=(e, st))
    de, dg, db = ops.bnact_bwd(e, n, h * w, c, st, gamma, 0, g=dz, partials=part)
    z = ef * st.scale + st.shift
    sg = torch.sigmoid(z)
    check(dz, da0.float() * (sg * (1 + z * (1 - sg))), 1.5e-2, "dZ0 (stride 2)")
    check(de, de_ref, 1.5e-2, "dE through the fused stride-2 epilogue")
    check(dg, dg_ref, 1e-2, "dgamma")
    check(db, db_ref, 1e-2, "dbeta")


def _bn_stats_of(e, c, seed):
    """BatchNorm statistics block of e [rows, c] with seeded gamma / beta (as the epilogue tests above build it)"""
    gamma, beta = rnd(c, seed=seed, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=seed + 1, dtype=torch.float32) * 0.1
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(e.shape[0])
    return st


def _check_bn_backward_epilogue(dz, part, da_ref, e, st, what):
    """dZ0 = dA0 * silu'(e * scale + shift) and the two BatchNorm-backward sums (sum dZ0, sum dZ0 * xhat0) against fp32 torch:
    da_ref [rows, c] is autograd's data gradient"""
    ef = e.float()
    z = ef * st.scale + st.shift
    sg = torch.sigmoid(z)
    dz_ref = da_ref * (sg * (1 + z * (1 - sg)))
    check(dz, dz_ref, 1.5e-2, what + ": dZ0")
    sums = part.double().sum(0)
    xhat = ((ef - st.mean) * st.invstd).double()
    check(sums[0].float(), dz_ref.double().sum(0).float(), 1e-2, what + ": sum dZ0 (dbeta)")
    check(sums[1].float(), (dz_ref.double() * xhat).sum(0).float(), 1e-2, what + ": sum dZ0 * xhat0 (dgamma)")


@pytest.mark.parametrize("k,s,pad,c", [(3, 1, (1, 1, 1, 1), 24), (3, 1, (1, 1, 1, 1), 72), (3, 2, (1, 1, 0, 1), 48), (5, 2, (2, 2, 1, 2), 40)])
def test_dwconv_marching_several_items_per_workgroup(k, s, pad, c):
    """The marching kernels' persistent loop past its first item: many small images, so that every workgroup owns two or more
    items (asserted through the work split: stat rows = workgroups per channel tile <= n / 2 <= items / 2) of several staged
    blocks each (h = 20).  That exercises the hand-over between items (accumulators and output pointer reset at block 0) and
    the prefetch of the next item's first block while the current item finishes.  Forward with prologue and statistics, weight
    gradient, stride-1 data gradient with the BatchNorm-backward epilogue, stride-2 data gradient with and without it; 6-lane
    tiles (c = 24), a ragged second 64-channel tile (c = 72), 48-channel tiles and the 5x5 form.  Reference: fp32 torch conv2d +
    autograd on the 16-bit-rounded operands; tolerances of test_dwconv_fwd / test_dwconv_bwd and of the epilogue tests.  (The
    stride-2 pads are the static "same" pads of a 20 x 9 map: odd width symmetric, even height one-sided.)"""
    import ctypes as C
    n, h, w = 1000, 20, 9
    Lh = L.load()
    x = rnd(n, h, w, c, seed=51)
    wt = rnd(c, 1, k, k, seed=52, dtype=torch.float32) * 0.3
    st = _bn_stats_of(x.view(-1, c), c, 53)
    pro = (st.scale, st.shift)
    a = F.silu(x.float() * pro[0] + pro[1]).to(BF).float().permute(0, 3, 1, 2).requires_grad_(True)
    wr = wt.clone().requires_grad_(True)
    ref = F.conv2d(F.pad(a, pad), wr, None, s, 0, 1, c)
    oh, ow = ref.shape[2], ref.shape[3]
    dy = rnd(n, oh, ow, c, seed=54)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    w_kkc = wt.view(c, k * k).t().contiguous()
    geo = (n, h, w, c, k, s, pad[0], pad[2], oh, ow)
    old = Lh.mc_dwconv_set_lane_mode(0)
    try:
        assert Lh.mc_dwconv_stat_rows(C.byref(ops._dw_args(*geo))) <= n // 2, "every workgroup needs a second item"
        y, part = ops.dwconv_fwd(x.view(-1, c), w_kkc, *geo, pro=pro, stats=True)
        check(y.view(n, oh, ow, c).permute(0, 3, 1, 2), ref.detach(), 1e-2, "dw fwd")
        sums, yf = part.double().sum(0), y.float().double()
        check(sums[0].float(), yf.sum(0).float(), 1e-4, "dw colsum")
        check(sums[1].float(), (yf * yf).sum(0).float(), 1e-4, "dw colsumsq")
        dw = ops.dwconv_bwd_weight(x.view(-1, c), dy.view(-1, c), *geo, pro=pro)
        check(dw.t().reshape(c, 1, k, k), wr.grad, 2e-3, "dw bwd weight")
        da_ref = a.grad.permute(0, 2, 3, 1).reshape(-1, c)
        if s == 1:
            w_flip = wt.flip(2, 3).reshape(c, k * k).t().contiguous()
            dz, part = ops.dwconv_bwd_data(dy.view(-1, c), w_kkc, *geo, w_kkc_flipped=w_flip, epi=(x.view(-1, c), st))
            assert part.shape[0] <= n // 2
            _check_bn_backward_epilogue(dz, part, da_ref, x.view(-1, c), st, "stride-1 dgrad")
        else:
            assert Lh.mc_dwconv_bwd_data_stat_rows(C.byref(ops._dw_args(*geo))) <= n // 2, "every workgroup needs a second item"
            dx = ops.dwconv_bwd_data(dy.view(-1, c), w_kkc, *geo)
            check(dx, da_ref, 1e-2, "stride-2 dgrad")
            dz, part = ops.dwconv_bwd_data(dy.view(-1, c), w_kkc, *geo, epi=(x.view(-1, c), st))
            _check_bn_backward_epilogue(dz, part, da_ref, x.view(-1, c), st, "stride-2 dgrad")
    finally:
        Lh.mc_dwconv_set_lane_mode(old)


@pytest.mark.parametrize("k,n,h,w,c,pad", [(3, 2, 140, 70, 72, (0, 1)), (5, 1, 141, 71, 40, (1, 2))])
def test_dwconv_s2_dgrad_row_segments_and_strips(k, n, h, w, c, pad):
    """Stride-2 data gradient, plain and with the BatchNorm-backward epilogue, on one tall and wide map: several column strips
    and several row segments per image (asserted through mc_dwconv_bwd_data_plan), so neighbouring segments meet across their
    D - 1 halo rows of dy and strips across their halo columns.  Reference: autograd of the fp32 torch conv2d."""
    import ctypes as C
    pl, pt = pad
    oh, ow = (h + 1) // 2, (w + 1) // 2
    plan = (C.c_int * 4)()
    assert L.load().mc_dwconv_bwd_data_plan(C.byref(ops._dw_args(n, h, w, c, k, 2, pl, pt, oh, ow)), plan) > 0
    assert plan[0] > 1 and plan[1] > 1, f"strips {plan[0]}, segments {plan[1]}"
    e = rnd(n * h * w, c, seed=61)
    dd = rnd(n * oh * ow, c, seed=62)
    wt = rnd(c, 1, k, k, seed=63, dtype=torch.float32) * 0.3
    st = _bn_stats_of(e, c, 64)
    a = torch.zeros(n, c, h, w, device=DEV, requires_grad=True)
    full = (pl, (ow - 1) * 2 + k - w - pl, pt, (oh - 1) * 2 + k - h - pt)
    F.conv2d(F.pad(a, full), wt, None, 2, 0, 1, c).backward(dd.float().view(n, oh, ow, c).permute(0, 3, 1, 2))
    da_ref = a.grad.permute(0, 2, 3, 1).reshape(-1, c)
    w_kkc = wt.view(c, k * k).t().contiguous()
    dx = ops.dwconv_bwd_data(dd, w_kkc, n, h, w, c, k, 2, pl, pt, oh, ow)
    check(dx, da_ref, 1e-2, "stride-2 dgrad")
    dz, part = ops.dwconv_bwd_data(dd, w_kkc, n, h, w, c, k, 2, pl, pt, oh, ow, epi=(e, st))
    _check_bn_backward_epilogue(dz, part, da_ref, e, st, "stride-2 dgrad")


@pytest.mark.parametrize("n_img,hw,cexp,cout", [(4, 4096, 240, 40), (3, 6016, 144, 40), (5, 2048, 24, 24), (2, 16384, 48, 24),  # (the model fuses from 192 channels up)
                                                (6, 1600, 96, 16), (2, 8192, 256, 64), (2, 4096, 144, 24), (3, 2736, 208, 32), (2, 4112, 176, 128)])
def test_proj_dgrad_with_se_and_bn1_backward_epilogues(n_img, hw, cexp, cout):
    """gemm_rows epi_mode 1 / 2: the projection conv's data gradient G = dP . Wp with the squeeze-excite sums / the
    BatchNorm1 + swish backward apply in its epilogue == linear_dgrad -> bnact_se_sums / bnact_bwd on the stored G
    (same bf16 rounding of G, same elementwise arithmetic; the sums differ only in summation order)."""
    M = n_img * hw
    assert ops.proj_dgrad_fusable(M, 256, cout, hw) and L.load().mc_gemm_rows_supported(cexp, cout)
    dp = rnd(M, cout, seed=1)
    d = rnd(M, cexp, seed=2)
    wp = rnd(cout, cexp, seed=3, scale=0.3)
    wp_t = wp.t().contiguous()
    gamma, beta = rnd(cexp, seed=4, dtype=torch.float32) * 0.2 + 1.0, rnd(cexp, seed=5, dtype=torch.float32) * 0.1
    df = d.float()
    mean, var = df.mean(0), df.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(M)
    gate = torch.sigmoid(rnd(n_img, cexp, seed=6, dtype=torch.float32))
    dpooled = rnd(n_img, cexp, seed=7, dtype=torch.float32)
    da1 = ops.linear_dgrad(dp, wp, w_t=wp_t)
    sums_ref = ops.bnact_se_sums(d, da1, n_img, hw, cexp, st, 1)
    sums = ops.proj_dgrad_se_sums(dp, wp_t, d, st, n_img, hw)
    for k in range(5):
        check(sums[k], sums_ref[k], 2e-5, f"se sums[{k}] through the dgrad epilogue")
    part = ops.bn_partials_from_se_sums(sums_ref, gate, dpooled, 1.0 / hw)
    dd_ref, dg_ref, db_ref = ops.bnact_bwd(d, n_img, hw, cexp, st, gamma, 1, g=da1, mul=gate, add=dpooled, add_scale=1.0 / hw, partials=part)
    coef, dg, db = ops.bn_bwd_coefs(part, M, st, gamma)
    dd = ops.proj_dgrad_bn_apply(dp, wp_t, d, st, coef, gate, dpooled, 1.0 / hw, hw)
    assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
    check(dd, dd_ref, 4e-3, "BatchNorm1 + swish backward through the dgrad epilogue")          # (one bf16 ulp: the FMA contraction may differ)
    assert float((dd.float() - dd_ref.float()).abs().max()) <= 2 ** -7 * float(dd_ref.float().abs().max())


# ------------------------------------------------------------------------------------------- fused attention
def _attn_inputs(b, t, nh, seed):
    H = nh * 64
    qkv = rnd(b * t, 3 * H, seed=seed, scale=1.5)
    mask = torch.ones(b, t, dtype=torch.long, device=DEV)
    for i in range(b):
        mask[i, t - (i * 7) % (t // 2):] = 0 if (i * 7) % (t // 2) else 1          # ragged report lengths
    maskb = ops.mask_bias(mask)
    dctx = rnd(b * t, H, seed=seed + 1)
    return qkv, mask, maskb, dctx


def _attn_torch(qkv, mask, dctx, b, t, nh, keep=None, p=0.0):
    """fp32 reference of BertSelfAttention's core on the same bf16 operands (keep = dropout keep mask [b,nh,t,t])."""
    H = nh * 64
    x = qkv.float().requires_grad_(True)
    q, k, v = (x[:, i * H:(i + 1) * H].view(b, t, nh, 64).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * 0.125 + (1 - mask.float())[:, None, None, :] * torch.finfo(torch.float32).min
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep / (1 - p)
    ctx = (pr @ v).permute(0, 2, 1, 3).reshape(b * t, H)
    ctx.backward(dctx.float())
    return ctx.detach(), x.grad


@pytest.mark.parametrize("b,t,nh", [(3, 256, 12), (5, 64, 12), (2, 32, 2), (4, 128, 3), (2, 224, 4)])
def test_fused_attention_vs_torch(b, t, nh):
    """fused QK^T -> mask -> softmax -> PV kernel and its backward against fp32 torch on the same operands"""
    assert ops.attn_supported(t, 64)
    qkv, mask, maskb, dctx = _attn_inputs(b, t, nh, 300 + t)
    ctx, lse = ops.attn_fwd(qkv, maskb, b, t, nh, 0.125, 0.0, 1, 0)
    ref, dref = _attn_torch(qkv, mask, dctx, b, t, nh)
    check(ctx, ref, 1e-2, "attention context")
    dqkv = ops.attn_bwd(qkv, maskb, dctx, lse, b, t, nh, 0.125, 0.0, 1, 0)
    H = nh * 64
    for i, nm in enumerate("QKV"):
        check(dqkv[:, i * H:(i + 1) * H], dref[:, i * H:(i + 1) * H], 1.5e-2, "attention d" + nm)
    # masked keys get no gradient through K / V
    dead = (mask == 0).view(-1)
    if dead.any():
        assert float(dqkv[dead][:, H:].float().abs().max()) == 0.0


@pytest.mark.parametrize("b,t,nh", [(2, 32, 1), (3, 64, 2)])
def test_fused_attention_mask_with_holes(b, t, nh):
    """the padded kernels take the key bias of an ARBITRARY mask, not a length: zeros at the start and in the middle of a
    row (key 0 kept), one row all ones; one and two key blocks"""
    H = nh * 64
    qkv, dctx = rnd(b * t, 3 * H, seed=500 + t, scale=1.5), rnd(b * t, H, seed=501 + t)
    mask = torch.ones(b, t, dtype=torch.long, device=DEV)
    mask[0, 1:5] = 0                                   # start of the row
    mask[0, t // 2 - 3:t // 2 + 6] = 0                 # middle (t = 64: across the key-block boundary)
    if b > 2:                                          # row 1 stays all ones
        mask[2, 2::3] = 0
        mask[2, t - 7:] = 0
    assert bool((mask[:, 0] == 1).all()) and bool((mask[1] == 1).all()) and not bool((mask[0] == 1).all())
    maskb = ops.mask_bias(mask)
    ctx, lse = ops.attn_fwd(qkv, maskb, b, t, nh, 0.125, 0.0, 1, 0)
    ref, dref = _attn_torch(qkv, mask, dctx, b, t, nh)
    check(ctx, ref, 1e-2, "attention context, mask with holes")
    dqkv = ops.attn_bwd(qkv, maskb, dctx, lse, b, t, nh, 0.125, 0.0, 1, 0)
    for i, nm in enumerate("QKV"):
        check(dqkv[:, i * H:(i + 1) * H], dref[:, i * H:(i + 1) * H], 1.5e-2, "attention d%s, mask with holes" % nm)
    dead = (mask == 0).view(-1)
    assert float(dqkv[dead][:, H:].float().abs().max()) == 0.0          # masked keys: exactly zero dK / dV


@pytest.mark.parametrize("b,t,nh", [(3, 256, 12), (4, 64, 2)])
def test_fused_attention_dropout_matches_unfused_kernels(b, t, nh):
    """same (seed, stream, element) dropout function as mc_softmax_fwd: the fused kernels reproduce the unfused
    batched-GEMM + softmax path mask for mask, forward and backward"""
    H, M, hd, p, seed, sid = nh * 64, b * t, 64, 0.1, 1234, 16
    qkv, mask, maskb, dctx = _attn_inputs(b, t, nh, 400 + t)
    ctx, lse = ops.attn_fwd(qkv, maskb, b, t, nh, 0.125, p, seed, sid)
    dqkv = ops.attn_bwd(qkv, maskb, dctx, lse, b, t, nh, 0.125, p, seed, sid)
    # unfused kernels (the path taken for shapes the fused kernel does not cover)
    scores = torch.empty((b, nh, t, t), dtype=torch.float32, device=DEV)
    ops.gemm(qkv, qkv[:, H:], scores, t, t, hd, 3 * H, 3 * H, t, c_f32=1, batch=b * nh, nb2=nh,
             sA=(t * 3 * H, hd), sB=(t * 3 * H, hd), sC=(nh * t * t, t * t), bias=maskb, bias_stride1=t, alpha=0.125)
    probs, pd = ops.softmax_fwd(scores, p, seed, sid)
    ctx2 = torch.empty((M, H), dtype=BF, device=DEV)
    ops.gemm(pd, qkv[:, 2 * H:], ctx2, t, hd, t, t, 3 * H, H, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * H, hd))
    check(ctx, ctx2, 4e-3, "fused vs unfused context (same dropout mask)")
    keep = (pd.float() > 0) | (probs.float() == 0)
    ref, dref = _attn_torch(qkv, mask, dctx, b, t, nh, keep=keep.float(), p=p)
    check(ctx, ref, 1.5e-2, "dropout attention context vs torch")
    dpd = torch.empty((b, nh, t, t), dtype=torch.float32, device=DEV)
    ops.gemm(dctx, qkv[:, 2 * H:], dpd, t, t, hd, H, 3 * H, t, c_f32=1, batch=b * nh, nb2=nh,
             sA=(t * H, hd), sB=(t * 3 * H, hd), sC=(nh * t * t, t * t))
    dq2 = torch.empty((M, 3 * H), dtype=BF, device=DEV)
    ops.gemm(pd, dctx, dq2[:, 2 * H:], t, hd, t, t, H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * H, hd), sC=(t * 3 * H, hd))
    ds = ops.softmax_bwd(probs, dpd, p, seed, sid, 0.125)
    ops.gemm(ds, qkv[:, H:], dq2, t, hd, t, t, 3 * H, 3 * H, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * 3 * H, hd))
    ops.gemm(ds, qkv, dq2[:, H:], t, hd, t, t, 3 * H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * 3 * H, hd))
    for i, nm in enumerate("QKV"):
        check(dqkv[:, i * H:(i + 1) * H], dq2[:, i * H:(i + 1) * H], 6e-3, "fused vs unfused d" + nm)
        check(dqkv[:, i * H:(i + 1) * H], dref[:, i * H:(i + 1) * H], 2e-2, "dropout attention d%s vs torch" % nm)


def test_fused_attention_rejects_unsupported_shapes():
    assert not ops.attn_supported(48, 64) and not ops.attn_supported(512, 64) and not ops.attn_supported(64, 32)
    qkv, mask, maskb, dctx = _attn_inputs(1, 32, 1, 9)
    with pytest.raises(mammo_clip_amd.lib.MammoClipHipError):
        ops.attn_fwd(qkv[:24], maskb[:, :24].contiguous(), 1, 24, 1, 0.125, 0.0, 1, 0)


# ------------------------------------------------------------------------------------------- folded BatchNorm backward
@pytest.mark.parametrize("n_img,hw,cin,cexp,skip,mean_shift", [
    (4, 4096, 40, 240, True, 0.0),        # streaming kernels (M >= ROWS_MIN_M)
    (2, 8208, 24, 144, False, 1.5),       # inputs with a large mean: the centred scatter matrix has to absorb it
    (3, 1392, 304, 1824, True, 0.5),      # late stage: tiled GEMMs
    (2, 2784, 512, 3072, False, 0.0),
])
def test_bn_fold_expand_backward(n_img, hw, cin, cexp, skip, mean_shift):
    """Backward of x -> e = x We^T -> bn0(e) from dZ alone (ops.bn_fold_expand_bwd) against fp32 autograd through
    conv + training-mode BatchNorm on the same bf16 operands, and against the explicit path it replaces
    (BatchNorm apply pass -> de, then the two gradient GEMMs)."""
    M = n_img * hw
    x = (rnd(M, cin, seed=501) .float() + mean_shift).to(BF)
    we = (rnd(cexp, cin, seed=502, dtype=torch.float32) * cin ** -0.5).contiguous()
    gamma = rnd(cexp, seed=503, dtype=torch.float32).abs() + 0.5
    beta = rnd(cexp, seed=504, dtype=torch.float32)
    dz = rnd(M, cexp, seed=505)
    dy = rnd(M, cin, seed=506) if skip else None
    web = ops.cast_bf16(we)
    e, part = ops.linear_fwd(x, web, stats=True)
    st = ops.bn_finalize(part, M, gamma, beta, torch.zeros(cexp, device=DEV), torch.ones(cexp, device=DEV), 0.01, 1e-3, False)
    # reduction partials of (dz, dz * xhat) the way the depthwise data-gradient epilogue leaves them: [rows, 2, c]
    xhat = (e.float() - st.mean) * st.invstd
    part0 = torch.stack([dz.float().sum(0), (dz.float() * xhat).sum(0)])[None].contiguous()
    coef, dg, db = ops.bn_bwd_coefs(part0, M, st, gamma)
    dx, dwe = ops.bn_fold_expand_bwd(dz, x, we, web, coef, db, M, residual=dy)
    # (a) fp32 autograd: e from the bf16 operands in fp32, BatchNorm with batch statistics
    xr = x.float().requires_grad_(True)
    wr = web.float().requires_grad_(True)
    er = xr @ wr.t()
    zr = F.batch_norm(er, None, None, gamma, beta, True, 0.0, 1e-3)
    zr.backward(dz.float())
    ref_dx = xr.grad + (dy.float() if skip else 0)
    check(dx, ref_dx, 1.5e-2, "folded dx vs autograd")
    check(dwe, wr.grad, 1.5e-2, "folded dWe vs autograd")
    # (b) the explicit path: apply pass writes de (bf16), then dgrad / wgrad GEMMs over de
    de, dg2, db2 = ops.bnact_bwd(e, n_img, hw, cexp, st, gamma, 0, g=dz, partials=part0)
    dx2 = ops.linear_dgrad(de, web, residual=dy, w_t=ops.cast_transpose_bf16(we))
    dwe2 = ops.linear_wgrad(de, x)
    assert relerr(dx, ref_dx) <= 1.5 * relerr(dx2, ref_dx) + 2e-3, (relerr(dx, ref_dx), relerr(dx2, ref_dx))
    assert relerr(dwe, wr.grad) <= 1.5 * relerr(dwe2, wr.grad) + 2e-3, (relerr(dwe, wr.grad), relerr(dwe2, wr.grad))
    print("fold", (n_img, hw, cin, cexp), "dx err", relerr(dx, ref_dx), "explicit", relerr(dx2, ref_dx),
          "dWe err", relerr(dwe, wr.grad), "explicit", relerr(dwe2, wr.grad))


def test_gemm_rows_bias():
    x = rnd(40000, 40, seed=510)
    w = rnd(40, 40, seed=511, scale=0.2)
    bias = rnd(40, seed=512, dtype=torch.float32)
    r = rnd(40000, 40, seed=513)
    y = ops.linear_fwd(x, w, bias=bias, residual=r)
    check(y, x.float() @ w.float().t() + bias + r.float(), 1e-2, "rows gemm + bias + residual")
    y2 = ops.linear_fwd(x, w, bias=bias)
    check(y2, x.float() @ w.float().t() + bias, 1e-2, "rows gemm + bias")


def test_bnact_bwd_reduce_with_dz_store():
    """the stride-2 blocks' one-pass form: dz = g * silu'(bn(x)) stored + (sum dz, sum dz*xhat) partials"""
    n_img, hw, c = 3, 1000, 144
    x = rnd(n_img * hw, c, seed=520)
    g = rnd(n_img * hw, c, seed=521)
    gamma = rnd(c, seed=522, dtype=torch.float32).abs() + 0.5
    beta = rnd(c, seed=523, dtype=torch.float32)
    xf = x.float()
    mean, var = xf.mean(0), xf.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale, st.shift = (gamma * st.invstd).contiguous(), (beta - mean * gamma * st.invstd).contiguous()
    dz, part = ops.bnact_bwd_reduce_dz(x, n_img, hw, c, st, 1, g)
    zr = (xf * st.scale + st.shift).requires_grad_(True)
    F.silu(zr).backward(g.float())
    check(dz, zr.grad, 1e-2, "dz")
    sums = part.sum(0)
    check(sums[0], zr.grad.sum(0), 2e-3, "sum dz")
    check(sums[1], (zr.grad * (xf - mean) * st.invstd).sum(0), 2e-3, "sum dz*xhat")
    # the plain reduce pass leaves the same partials and stores nothing
    de, dg, db = ops.bnact_bwd(x, n_img, hw, c, st, gamma, 1, g=g)
    check(db, sums[0], 1e-5, "dbeta == sum dz")


# ------------------------------------------------------------------------------------------------ round 6: expand conv inside the depthwise launch
XDW_CASES = [  # k, s, n, h, w, cin, c: strips / image groups / ragged channel tiles / all three K-chunk instances (cin <= 32, 64, 128)
    (3, 1, 2, 70, 300, 40, 240), (3, 2, 2, 77, 131, 24, 144), (5, 2, 2, 120, 250, 40, 240), (5, 1, 3, 150, 130, 64, 384),
    (3, 2, 3, 61, 95, 64, 384), (3, 1, 5, 95, 57, 128, 768), (5, 1, 3, 48, 57, 128, 200), (5, 1, 9, 48, 29, 48, 288),
    (3, 1, 9, 7, 9, 16, 96), (5, 2, 3, 9, 11, 24, 144), (5, 1, 2, 33, 70, 88, 528), (3, 1, 1, 20, 20, 8, 48)]


@pytest.mark.parametrize("k,s,n,h,w,cin,c", XDW_CASES)
def test_mbconv_xdw_fused_expand_depthwise(k, s, n, h, w, cin, c):
    """mc_mbconv_xdw_fwd (conv_lane.hip MODE 4): expand 1x1 conv -> BatchNorm0 + swish -> depthwise conv in one launch
    [ref: efficientnet_custom.py:104-111] against (a) the fp32 torch composition and (b) the two launches it replaces.  The
    fused launch does not round e to 16 bits before BatchNorm0 (the two-launch form does): (b) is therefore a closeness
    check at the 16-bit rounding level, not bit equality; the BatchNorm1 statistics partials must be the sums of the STORED
    output."""
    pad = (k - 1) // 2 if s == 1 else (k - 2) // 2
    oh, ow = (h + s - 1) // s, (w + s - 1) // s
    x = rnd(n * h * w, cin, seed=41)
    we = rnd(c, cin, seed=42, scale=cin ** -0.5)
    wk = rnd(k * k, c, seed=43, dtype=torch.float32) * 0.3
    pro = (rnd(c, seed=44, dtype=torch.float32) * 0.3 + 1.0, rnd(c, seed=45, dtype=torch.float32) * 0.3)
    assert ops.mbconv_xdw_ok(n, h, w, cin, c, k, s, pad, pad, oh, ow)
    y, part = ops.mbconv_xdw_fwd(x, we, pro, wk, n, h, w, c, k, s, pad, pad, oh, ow, stats=True)
    torch.cuda.synchronize()
    # (a) fp32 reference: activations rounded to 16 bits where the kernel rounds them (the staged tile), nothing else
    e = x.float() @ we.float().T
    a0 = F.silu(e * pro[0] + pro[1]).to(BF).float().view(n, h, w, c).permute(0, 3, 1, 2)
    wt = wk.t().contiguous().view(c, 1, k, k)
    ref = F.conv2d(F.pad(a0, (pad, k - 1 - pad + (s - 1), pad, k - 1 - pad + (s - 1))), wt, None, s, 0, 1, c)[:, :, :oh, :ow]
    check(y.view(n, oh, ow, c).permute(0, 3, 1, 2), ref, 1e-2, "xdw vs fp32 torch")
    # (b) the two launches: e rounded to 16 bits in between
    e16 = ops.linear_fwd(x, we)
    y2 = ops.dwconv_fwd(e16, wk, n, h, w, c, k, s, pad, pad, oh, ow, pro=pro)
    check(y, y2, 2e-2, "xdw vs expand GEMM + depthwise launch")
    st = part.double().sum(0)
    yf = y.float().double()
    check(st[0].float(), yf.sum(0).float(), 1e-4, "xdw colsum")
    check(st[1].float(), (yf * yf).sum(0).float(), 1e-4, "xdw colsumsq")


def test_mbconv_xdw_identity_weights_asymmetric_input():
    """A = I check of the MFMA staging (operand / accumulator layout, pixel -> LDS position, zero padding): with the expand
    weight a 0/1 selection matrix and BatchNorm0 the identity, the fused launch must equal the plain depthwise launch on the
    selected channels BIT FOR BIT (silu is applied to exactly representable values in both)."""
    k, s, n, h, w, cin, c = 3, 1, 2, 37, 131, 32, 64
    x = rnd(n * h * w, cin, seed=51)
    sel = torch.arange(c, device=DEV) * 7 % cin                 # asymmetric: expanded channel i reads input channel 7 i mod cin
    we = torch.zeros(c, cin, device=DEV)
    we[torch.arange(c, device=DEV), sel] = 1.0
    we = we.to(BF)
    wk = rnd(k * k, c, seed=53, dtype=torch.float32) * 0.3
    one, zero = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    y = ops.mbconv_xdw_fwd(x, we, (one, zero), wk, n, h, w, c, k, s, 1, 1, h, w)
    y2 = ops.dwconv_fwd(x[:, sel].contiguous(), wk, n, h, w, c, k, s, 1, 1, h, w, pro=(one, zero))
    assert torch.equal(y, y2)


@pytest.mark.parametrize("rows,cin,c,shift", [(20000, 40, 240, 0.0), (9000, 24, 144, 3.0), (12000, 64, 384, -1.5), (8200, 128, 768, 0.5)])
def test_bn_statistics_from_the_gram_matrix(rows, cin, c, shift):
    """mc_bn_gram_partials: training-mode BatchNorm statistics of e = x W^T from x^T x and colsum(x) alone, against fp64
    statistics of the fp32 product (the tensor the fused launch normalises -- never rounded to 16 bits), including inputs
    whose mean dominates their spread (mean^2 >> var on many channels)."""
    x = (rnd(rows, cin, seed=61, dtype=torch.float32) + shift).to(BF)
    we = rnd(c, cin, seed=62, scale=cin ** -0.5)
    part, (xtx, cs) = ops.bn_gram_partials(x, we, rows)
    check(cs, x.float().sum(0), 1e-4, "colsum")
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    st = ops.bn_finalize(part, rows, gamma, beta, rm, rv, 0.01, 1e-3, True)
    e = x.double() @ we.double().T
    mean, var = e.mean(0), e.var(0, unbiased=False)
    assert float((st.mean.double() - mean).abs().max()) <= 1e-5 * float(mean.abs().max() + 1.0)
    invstd = 1.0 / torch.sqrt(var + 1e-3)
    assert float((st.invstd.double() / invstd - 1.0).abs().max()) <= 2e-5
    assert float((rm.double() - 0.01 * mean).abs().max()) <= 1e-6 * float(mean.abs().max() + 1.0)
    assert float((rv.double() - (0.99 + 0.01 * e.var(0, unbiased=True))).abs().max()) <= 1e-5 * float(var.max() + 1.0)


XE_CASES = [  # n, h, w, cin, c: strips (w > 62), image groups, ragged channel tiles, both K-chunk instances (cin <= 32 / 64)
    (2, 70, 300, 40, 240), (3, 33, 59, 24, 144), (5, 95, 57, 64, 72), (33, 48, 29, 16, 96), (9, 7, 9, 8, 24), (1, 200, 62, 48, 40),
    (2, 41, 130, 64, 384)]


@pytest.mark.parametrize("n,h,w,cin,c", XE_CASES)
def test_dwconv_fused_backward_with_e_rows_formed_from_the_block_input(n, h, w, cin, c):
    """Round 6 (conv_lane.hip MODE 5): mc_dwconv_bwd_fused with xw -- the launch forms the e rows it needs (silu'(bn0(e)), the
    BatchNorm0 reductions, a0 = silu(bn0(e)) of the weight gradient) from the block input x and the expand weight by the MFMA
    staging of the fused forward, instead of reading e [ref: efficientnet_custom.py:104-111 backwards].  Against the same launch
    reading e = the expand GEMM's stored output: the staged e is the same fp32 accumulation rounded once to 16 bits, so dZ0,
    the partials and dW agree to the last-bit spread of two MFMA accumulation orders (<= 2 units of 16-bit rounding on dZ0
    where an e value differs, which moves silu' by <= 1e-2 relative)."""
    k, pad = 3, 1
    x = rnd(n * h * w, cin, seed=71)
    we = rnd(c, cin, seed=72, scale=cin ** -0.5)
    dd = rnd(n * h * w, c, seed=73)
    wk = rnd(k * k, c, seed=74, dtype=torch.float32)
    gamma, beta = rnd(c, seed=75, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=76, dtype=torch.float32) * 0.1
    e = ops.linear_fwd(x, we)
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(n * h * w)
    wflip = wk.flip(0).contiguous()
    assert ops.dwconv_bwd_fused_ok(n, h, w, c, k, 1, pad, pad, h, w, force=True, cin=cin)
    dz_ref, part_ref, dw_ref = ops.dwconv_bwd_fused(dd, e, st, wflip, n, h, w, c, k, pad, pad, h, w)
    for _ in range(2):
        dz, part, dw = ops.dwconv_bwd_fused(dd, None, st, wflip, n, h, w, c, k, pad, pad, h, w, xw=(x, we))
    torch.cuda.synchronize()
    assert torch.isfinite(dz.float()).all() and torch.isfinite(dw).all()
    frac_equal = float((dz == dz_ref).float().mean())
    check(dz, dz_ref, 1e-2, "dZ0 (e rows from x) vs dZ0 (e read)")
    assert frac_equal >= 0.98, frac_equal                   # almost every element bit-identical: the staged e IS the stored e
    s0, s1 = part_ref.double().sum(0), part.double().sum(0)
    scale = s0.abs().amax(dim=1, keepdim=True)
    assert float(((s0 - s1).abs() / scale).max()) <= 2e-3, "BatchNorm-backward partials"
    assert float((dw - dw_ref).abs().max()) <= 2e-3 * float(dw_ref.abs().max()), "dW"


def test_fused_launches_random_geometry_screen():
    """scripts/xdw_fuzz.py: 150 random geometries (kernel 3 / 5, stride 1 / 2 with the reference's symmetric and asymmetric static
    paddings, 1-17 images, maps from k x k to 90 x 320, cin 8-128, c 8-384) of the fused expand + depthwise forward against the two
    launches it replaces and fp32 torch, and of the fused backward with its e rows formed from the block input against the same
    launch reading the stored e."""
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "xdw_fuzz.py")
    r = subprocess.run([sys.executable, script, "150", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ past the grid caps
# Each shape is the smallest that leaves the first pass of its launcher's capped grid by one ragged workgroup (the caps are
# in the launchers of bert.hip / util.hip); references are fp64 torch on the 16-bit-rounded inputs the kernel reads.  Every
# op is called once per distinct input: the wrappers allocate their outputs, and a block handed back by the caching
# allocator could still hold an earlier, correct answer.
def check_late(got, ref, first, tol, what=""):
    """`check` on the whole tensor and on the part past the first pass (dim 0: rows, or the elements of a flat view), which
    is then normalised by its own max|ref|"""
    check(got, ref, tol, what)
    assert got.shape[0] > first, (what, got.shape, first)
    check(got[first:], ref[first:], tol, f"{what} [{first}:]")


def _add_ln_ref64(x, res, gamma, beta, dys):
    """fp64 LayerNorm(x + res) and, per upstream gradient in dys, the gradients of (x, res, gamma, beta)"""
    leaves = [v.double().requires_grad_(True) for v in (x, res, gamma, beta)]
    y = F.layer_norm(leaves[0] + leaves[1], (x.shape[1],), leaves[2], leaves[3], 1e-12)
    return y.detach(), [torch.autograd.grad(y, leaves, dy.double(), retain_graph=True) for dy in dys]


def test_add_ln_past_the_grid_cap():
    """forward: 2048 workgroups x 4 rows, 8197 rows = one 5-row second pass; backward: 512 workgroups x 4 rows, 4101 rows =
    three passes.  dgamma / dbeta of the later passes alone: dy zero in the rows of the first backward pass."""
    h, FWD, BWD = 768, 8192, 2048
    x, res = rnd(FWD + 5, h, seed=600), rnd(FWD + 5, h, seed=601)
    gamma, beta = rnd(h, seed=602, dtype=torch.float32) * 0.1 + 1, rnd(h, seed=603, dtype=torch.float32) * 0.1
    ref, _ = _add_ln_ref64(x, res, gamma, beta, [])
    y, mean, rstd = ops.add_ln_fwd(x, res, gamma, beta, 1e-12, 0.0, 1, 0)
    check_late(y, ref, FWD, 1e-2, "add_ln fwd")
    s = x.double() + res.double()
    check_late(mean, s.mean(1), FWD, 1e-4, "add_ln mean")
    check_late(rstd, (s.var(1, unbiased=False) + 1e-12).rsqrt(), FWD, 1e-4, "add_ln rstd")
    rows = 2 * BWD + 5
    xb, rb, mb, sb = x[:rows], res[:rows], mean[:rows], rstd[:rows]     # (per-row statistics: checked above)
    dy = rnd(rows, h, seed=604)
    dy0 = dy.clone()
    dy0[:BWD] = 0
    _, (g, g0) = _add_ln_ref64(xb, rb, gamma, beta, [dy, dy0])
    dx, dres, dgamma, dbeta = ops.add_ln_bwd(dy, xb, rb, gamma, mb, sb, 0.0, 1, 0)
    check_late(dx, g[0], BWD, 1.5e-2, "add_ln dx")
    check_late(dres, g[1], BWD, 1.5e-2, "add_ln dres")
    check(dgamma, g[2], 2e-3, "add_ln dgamma")
    check(dbeta, g[3], 2e-3, "add_ln dbeta")
    dx0, dres0, dgamma0, dbeta0 = ops.add_ln_bwd(dy0, xb, rb, gamma, mb, sb, 0.0, 1, 0)
    check(dgamma0, g0[2], 2e-3, "add_ln dgamma of passes two and three")
    check(dbeta0, g0[3], 2e-3, "add_ln dbeta of passes two and three")
    assert float(dx0[:BWD].float().abs().max()) == 0.0 and float(dres0[:BWD].float().abs().max()) == 0.0
    check(dx0[BWD:], g0[0][BWD:], 1.5e-2, "add_ln dx of passes two and three")
    check(dres0[BWD:], g0[1][BWD:], 1.5e-2, "add_ln dres of passes two and three")


def test_add_ln_dropout_past_the_grid_cap():
    """p = 0.1 at 8197 rows: the forward is bit-reproducible, and the mask the backward regenerates is the forward's, in the
    later passes of both (forward rows >= 8192, backward rows >= 2048)"""
    rows, h, p, FWD, BWD = 8197, 768, 0.1, 8192, 2048
    x, res = rnd(rows, h, seed=605), torch.zeros(rows, h, device=DEV, dtype=BF)
    gamma, beta = torch.ones(h, device=DEV), torch.zeros(h, device=DEV)
    y1, m1, r1 = ops.add_ln_fwd(x, res, gamma, beta, 1e-12, p, 77, 5)
    y2, _, _ = ops.add_ln_fwd(x, res, gamma, beta, 1e-12, p, 77, 5)           # (y1 is alive: y2 is another block)
    assert torch.equal(y1, y2)
    # forward mask: with res = 0, gamma = 1, beta = 0 the normalised row gives the dropped-out sum back, s = y / rstd + mean,
    # which is 0 where x was dropped and x / 0.9 where it was kept.  y carries one 16-bit rounding (<= 2^-9 |y|, |y| < 6,
    # 1 / rstd ~ 1), so s is known to 0.02: looked at where |x| > 0.25, kept is |s| > 0.27 - 0.02 and dropped is |s| < 0.02
    s = y1.float() / r1[:, None] + m1[:, None]
    bigx = x.float().abs() > 0.25
    keep_f = s.abs() > 0.12
    frac = float(keep_f[FWD:][bigx[FWD:]].float().mean())
    assert abs(frac - 0.9) < 0.02, frac
    dy = rnd(rows, h, seed=606)
    dx, dres, _, _ = ops.add_ln_bwd(dy, x, res, gamma, m1, r1, p, 77, 5)
    big = dres.float().abs() > 1e-3
    keep_b = dx.float().abs() > 0
    both = bigx & big
    assert torch.equal(keep_b[both], keep_f[both])
    assert int(both[FWD:].sum()) > 1000 and torch.equal(keep_b[FWD:][both[FWD:]], keep_f[FWD:][both[FWD:]])
    # the ratio check of test_add_ln_dropout_consistency on the rows of the later backward passes
    dxl, dresl, bigl = dx[BWD:].float(), dres[BWD:].float(), big[BWD:]
    sel = (dxl.abs() > 0) & bigl
    frac = float(sel.float().sum() / bigl.float().sum())
    assert abs(frac - 0.9) < 0.02, frac
    ratio = dxl[sel] / dresl[sel]
    assert float((ratio - 1 / 0.9).abs().max()) < 2e-2


def test_bert_embed_past_the_grid_cap():
    """33 x 249 = 8217 rows: a 25-row second forward pass; backward: 2048 / 249 = 8 batch rows per round, five rounds with
    one batch row in the last.  97 words: every word row collects ~85 atomic adds.  Second backward call: dy zero in batch
    rows < 8, so all five gradients come from rounds two to five alone."""
    b, t, h, vocab, FWD = 33, 249, 64, 97, 8192
    g = torch.Generator().manual_seed(610)
    ids = torch.randint(0, vocab, (b, t), generator=g).to(DEV)
    tt = torch.randint(0, 2, (b, t), generator=g).to(DEV)
    word, pos, typ = (rnd(n, h, seed=611 + i, dtype=torch.float32) for i, n in enumerate((vocab, 256, 2)))
    gamma, beta = rnd(h, seed=614, dtype=torch.float32) * 0.1 + 1, rnd(h, seed=615, dtype=torch.float32) * 0.1
    lv = [v.double().requires_grad_(True) for v in (word, pos, typ, gamma, beta)]
    ref = F.layer_norm(lv[0][ids] + lv[1][:t][None] + lv[2][tt], (h,), lv[3], lv[4], 1e-12)
    y, mean, rstd = ops.bert_embed_fwd(ids, tt, word, pos, typ, gamma, beta, 1e-12, 0.0, 1, 0)
    check_late(y, ref.detach().view(b * t, h), FWD, 1e-2, "embed fwd")
    dy = rnd(b * t, h, seed=616)
    dy0 = dy.clone()
    dy0[:8 * t] = 0
    for d, tag in ((dy, ""), (dy0, " of rounds two to five")):
        refs = torch.autograd.grad(ref, lv, d.double().view(b, t, h), retain_graph=True)
        got = ops.bert_embed_bwd(d, ids, tt, word, pos, typ, gamma, mean, rstd, 0.0, 1, 0)
        for a, r, nm in zip(got, refs, ("dword", "dpos", "dtype", "dgamma", "dbeta")):
            check(a, r, 2e-3, "embed " + nm + tag)


def test_gelu_past_the_grid_cap():
    """8192 workgroups x 256 lanes x 8 elements = 16,777,216 elements; 5464 x 3072 leaves 1024 vectors to a second pass"""
    rows, c, first = 5464, 3072, 8192 * 256 * 8
    x, dy = rnd(rows, c, seed=620), rnd(rows, c, seed=621)
    chunk = 683                                                  # fp64 in 8 pieces, kept as fp32 (2^-24: nothing beside 1e-2)
    ref = torch.cat([F.gelu(xc.double()).float() for xc in x.split(chunk)])
    check_late(ops.gelu_fwd(x).view(-1), ref.view(-1), first, 1e-2, "gelu")
    del ref

    def dgelu(xc):                                               # d/dx [x Phi(x)] = Phi(x) + x phi(x)
        xd = xc.double()
        return 0.5 * (1 + torch.erf(xd / math.sqrt(2))) + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
    refd = torch.cat([(dc.double() * dgelu(xc)).float() for xc, dc in zip(x.split(chunk), dy.split(chunk))])
    check_late(ops.gelu_bwd(dy, x).view(-1), refd.view(-1), first, 1e-2, "gelu bwd")


@pytest.mark.parametrize("rows,t,first", [(32771, 256, 32768),     # 8 keys per lane, 32 lanes per row: 4096 workgroups x 8 rows
                                          (16389, 40, 16384)])     # one key per lane-slot: 4096 workgroups x 4 rows
def test_softmax_past_the_grid_cap(rows, t, first):
    """test_softmax_fwd_bwd's masking, checks and bounds, one ragged workgroup past the first pass, against fp64"""
    live = (t * 3) // 4
    s = rnd(rows, t, seed=630, dtype=torch.float32) * 3
    s[:, live:] = -3.0e38
    sr = s.double().requires_grad_(True)
    ref = torch.softmax(sr, -1)
    probs, pd = ops.softmax_fwd(s, 0.0, 1, 0)
    assert pd.data_ptr() == probs.data_ptr()
    check_late(probs, ref.detach(), first, 1e-2, "softmax")
    dp = rnd(rows, t, seed=631, dtype=torch.float32)
    dpd = dp.double()
    ref.backward(dpd)
    refds = sr.grad * 0.125
    pq = ref.detach().float().to(BF)                             # the 16-bit probabilities the kernel sees
    pb = pq.double()
    refds2 = pb * (dpd - (pb * dpd).sum(-1, keepdim=True)) * 0.125
    ds = ops.softmax_bwd(pq, dp, 0.0, 1, 0, 0.125)
    check_late(ds, refds2, first, 1e-2, "softmax bwd")
    assert relerr(ds, refds) < 5e-2 and relerr(ds[first:], refds[first:]) < 5e-2
    if t % 8:
        return                                                   # dropout draws are per 8-element group
    probs2, pd2 = ops.softmax_fwd(s, 0.1, 5, 2)
    check_late(probs2, ref.detach(), first, 1e-2, "softmax (dropout call)")
    on = probs2[:, :live].float() > 0
    nz = float((pd2[:, :live].float() > 0)[on].float().mean())
    assert abs(nz - 0.9) < 0.03, nz
    # mask regeneration in the backward, evaluated on the rows past the first pass (and on all of them)
    keep = (pd2.double() > 0).double() / 0.9
    pb2 = probs2.double()
    refds3 = pb2 * (dpd * keep - (pb2 * dpd * keep).sum(-1, keepdim=True)) * 0.125
    ds3 = ops.softmax_bwd(probs2, dp, 0.1, 5, 2, 0.125)
    sel = pb2 > 1e-3                                             # where a dropped probability is distinguishable from 0
    err = (ds3.double() - refds3).abs()
    assert int(sel[first:].sum()) > 50
    assert float(err[first:][sel[first:]].max()) <= 2e-2 * float(refds3[first:].abs().max()) + 1e-3
    assert float(err[sel].max()) <= 2e-2 * float(refds3.abs().max()) + 1e-3


def test_casts_past_the_grid_cap_and_tails():
    """bit-exact against torch: cast_f32_bf16 (4096 workgroups x 2048 elements, then 2048 + 5: a second pass that ends in the
    scalar tail), the low-part cast and the widening cast (8192 x 256 elements, then 300), misaligned source, transpose"""
    x = rnd(4096 * 2048 + 2048 + 5, seed=640, dtype=torch.float32)
    assert torch.equal(ops.cast_bf16(x), x.to(BF))
    # a source at element offset 1 (4 bytes past a 16-byte boundary).  The wrapper's .contiguous() returns a 1-D slice as it
    # is, so the kernel does see the misaligned pointer and takes the scalar branch for both groups; n = 13 also ends in a
    # 5-element tail.  out= : no cached image
    base = rnd(16, seed=641, dtype=torch.float32)
    src = base[1:14]
    assert src.data_ptr() % 16 == 4
    out = torch.full((16,), 7.0, device=DEV, dtype=BF)
    ops.cast_bf16(src, out=out[:13])
    assert torch.equal(out[:13], src.to(BF)) and bool((out[13:].float() == 7.0).all())
    al = rnd(13, seed=642, dtype=torch.float32)                  # aligned: one vector, then the tail
    out = torch.full((16,), 7.0, device=DEV, dtype=BF)
    ops.cast_bf16(al, out=out[:13])
    assert torch.equal(out[:13], al.to(BF)) and bool((out[13:].float() == 7.0).all())
    x2 = rnd(8192 * 256 + 300, seed=643, dtype=torch.float32)
    hi = x2.to(BF)
    assert torch.equal(ops.cast_bf16_lo(x2), (x2 - hi.float()).to(BF))
    assert torch.equal(ops.cast_f32(hi), hi.float())
    m = rnd(70, 45, seed=644, dtype=torch.float32)               # 3 x 2 tiles of 32, ragged in both directions
    assert torch.equal(ops.cast_transpose_bf16(m), m.t().contiguous().to(BF))
    v = rnd(1000, seed=645, dtype=torch.float32)
    sd = torch.tensor([1.7], device=DEV)
    check(ops.scale_f32(v, alpha=0.5), v * 0.5, 1e-6, "scale_f32")
    check(ops.scale_f32(v, sd, 0.5), v * (torch.tensor(0.5, device=DEV) * sd), 1e-6, "scale_f32 scalar_dev")


def test_colsum_past_the_grid_cap():
    """c = 2048: one row per workgroup iteration, 16 rows per workgroup -> 513 workgroups capped at 512, so rows >= 8192 are a
    second pass.  Sums of the last / first eighth of the rows alone; accumulate into out=; row stride != c."""
    m, c = 8200, 2048
    assert L.load().mc_colsum_rows(m, c) == 512 and 512 * 16 < m
    x = rnd(m, c, seed=650)
    check(ops.colsum(x), x.double().sum(0), 1e-4, "colsum")
    late = x.clone()
    late[:m - m // 8] = 0
    check(ops.colsum(late), late.double().sum(0), 1e-4, "colsum, last eighth of the rows")
    early = x.clone()
    early[m // 8:] = 0
    check(ops.colsum(early), early.double().sum(0), 1e-4, "colsum, first eighth of the rows")
    out0 = rnd(c, seed=651, dtype=torch.float32) * 50
    out = out0.clone()
    assert ops.colsum(late, out=out, accumulate=True) is out
    check(out, out0.double() + late.double().sum(0), 1e-4, "colsum accumulate")
    w = rnd(m, 256, seed=652)
    check(ops.colsum(w[:, :240]), w[:, :240].double().sum(0), 1e-4, "colsum, row stride 256 != c")


# ------------------------------------------------------------------------------------------------ heads at product shapes
SGEMM_SHAPES = [(1, 1, 4), (1, 1, 33000), (33, 65, 100), (70, 512, 2048), (64, 512, 1024), (1024, 512, 32)]


def _sgemm_plan(m, n, k):
    """(S, L) of mc_sgemm's launch: S split-K partials (mc_sgemm_ws_floats = S * m * n, 0 when unsplit) and the longest
    serial accumulation chain L: k, or sgemm_k's k range per split, ceil(k / S) rounded up to the 32-wide k tile"""
    ws = L.load().mc_sgemm_ws_floats(m, n, k)
    S = ws // (m * n) if ws else 1
    kper = -(-(-(-k // S)) // 32) * 32
    return S, (kper if S > 1 else k)


@pytest.mark.parametrize("layout", ["nt", "tn"])
@pytest.mark.parametrize("m,n,k", SGEMM_SHAPES)
def test_sgemm_product_shapes(m, n, k, layout):
    """the layouts loss/_infonce.py, projection.py and evaluator.py call mc_sgemm with: dot product over b * D (32 splits),
    k = 4, k = batch, m / n across a 32-wide tile, split-K with beta = 1 through the finish kernel, alpha_dev, bias, ldc > n.

    Bound, per element, worst case for fp32 (u = 2^-24), so a correct kernel cannot miss it and a single-element result near
    zero (m = n = 1) is not divided by itself:
      * a chain of L fused multiply-adds rounds L times: |acc - sum a b| <= L u sum|a||b|             (first order in u)
      * the finish kernel adds S partials in order: S - 1 more roundings of partial sums, each <= sum|a||b|
      * alpha * acc rounds once (alpha itself = fp32(alpha) * alpha_dev is formed here exactly as the kernel forms it)
      => |alpha| (L + S) u (|A| @ |B|) = g |alpha| (|A| @ |B|),   g = (L + S) 2^-24,  L = k range per split (k when unsplit)
      * "+ bias" and "+ beta c" round once each, at most u times the magnitude of what they add up:
        + u (|alpha| |A| @ |B| + |bias| + |c|) per epilogue add."""
    assert sum(_sgemm_plan(*shp)[0] > 1 for shp in SGEMM_SHAPES) >= 2
    S, chain = _sgemm_plan(m, n, k)
    u = 2.0 ** -24
    g = (chain + S) * u
    A, B = rnd(m, k, seed=660, dtype=torch.float32), rnd(k, n, seed=661, dtype=torch.float32)
    if layout == "nt":                                           # a [m, k] and b [n, k] row-major: a @ b.T
        a_st, ars, acs, b_st, brs, bcs = A, k, 1, B.t().contiguous(), 1, k
    else:                                                        # a [k, m] and b [k, n] row-major: a.T @ b
        a_st, ars, acs, b_st, brs, bcs = A.t().contiguous(), 1, m, B, n, 1
    prod = A.double() @ B.double()
    mag = A.double().abs() @ B.double().abs()

    def within(got, ref, tol, what):
        assert torch.isfinite(got).all(), what + ": non-finite"
        excess = float(((got.double() - ref).abs() - tol).max())
        print(f"sgemm {layout} {m}x{n}x{k} S={S} L={chain} {what}: max err / bound "
              f"{float(((got.double() - ref).abs() / tol.clamp_min(1e-300)).max()):.3f}")
        assert excess <= 0.0, f"{what}: |err| exceeds the bound by {excess:.3e}"

    c = torch.full((m, n), float("nan"), device=DEV)
    ops.sgemm(a_st, ars, acs, b_st, brs, bcs, c, n, m, n, k)
    within(c, prod, g * mag, "plain")
    # device scalar x host alpha, bias; c = columns 2 .. 2 + n of a wider buffer, NaN there (beta = 0 must not read c)
    ldc = n + 5
    sd = torch.tensor([14.285], device=DEV)
    alpha = float((torch.tensor(0.5, device=DEV) * sd).double())
    bias = rnd(n, seed=662, dtype=torch.float32)
    wide = torch.full((m, ldc), 123.0, device=DEV)
    wide[:, 2:2 + n] = float("nan")
    ops.sgemm(a_st, ars, acs, b_st, brs, bcs, wide[:, 2:], ldc, m, n, k, alpha=0.5, bias=bias, alpha_dev=sd)
    amag = abs(alpha) * mag
    within(wide[:, 2:2 + n], alpha * prod + bias.double(), g * amag + u * (amag + bias.double().abs()), "alpha_dev + bias, ldc > n")
    assert bool((wide[:, :2] == 123.0).all()) and bool((wide[:, 2 + n:] == 123.0).all())
    # beta = 1 into a non-zero c (split shapes: through the finish kernel), ldc > n
    wide0 = rnd(m, ldc, seed=663, dtype=torch.float32)
    wide = wide0.clone()
    ops.sgemm(a_st, ars, acs, b_st, brs, bcs, wide[:, 2:], ldc, m, n, k, beta=1.0)
    c0 = wide0[:, 2:2 + n].double()
    within(wide[:, 2:2 + n], prod + c0, g * mag + u * (mag + c0.abs()), "beta = 1, ldc > n")
    assert torch.equal(wide[:, :2], wide0[:, :2]) and torch.equal(wide[:, 2 + n:], wide0[:, 2 + n:])


CE_CASES = [(r, n) for r in (1, 5, 300) for n in (1, 64, 65, 200, 1000) if r <= n]     # (the arange labels must fit)


def _ce_ref64(logits, labels, w, smoothing):
    lg = logits.double().requires_grad_(True)
    loss = w * F.cross_entropy(lg, labels, label_smoothing=smoothing)
    loss.backward()
    return loss.detach(), lg.grad


def _check_dlogits(got, ref, scale, what):
    """the file's 1e-4 of max|ref|, plus the rounding floor of (p - target - eps / n) * scale: three terms <= 1 held in fp32
    cancel to +-4 * 2^-24 at best.  That is 0.25 % of the bound wherever max|ref| ~ scale; it matters for n = 1 only, where
    the exact gradient is 0 and a bound relative to max|ref| = 0 would ask for an exact cancellation."""
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err, bound = float((got.double() - ref).abs().max()), 1e-4 * float(ref.abs().max()) + 4 * 2.0 ** -24 * scale
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("rows,n", CE_CASES)
def test_ce_fwd_bwd_shapes(rows, n, smoothing):
    """one wave per row strides the n columns by 64, one workgroup sums the row losses by 256: n = 1 / 64 / 65 / 200 / 1000,
    rows = 1 / 5 / 300, logits within +-30 (what logit_scale reaches), against fp64 F.cross_entropy"""
    w = 0.25
    logits = 30 * torch.tanh(rnd(rows, n, seed=670, dtype=torch.float32))
    off = (n - rows) // 2
    lref, gref = _ce_ref64(logits, torch.arange(rows, device=DEV) + off, w, smoothing)
    buf, loss = logits.clone(), torch.zeros(1, device=DEV)
    ops.ce_fwd_bwd(buf, off, w, loss, smoothing=smoothing)
    check(loss[0], lref, 1e-5, "ce loss, arange labels")
    _check_dlogits(buf, gref, w / rows, "ce dlogits, arange labels")
    # explicit labels (a permutation), the loss added into a slot that already holds 3.5
    labels = torch.randperm(n, generator=torch.Generator().manual_seed(671))[:rows].to(DEV)
    lref, gref = _ce_ref64(logits, labels, w, smoothing)
    buf, loss = logits.clone(), torch.full((1,), 3.5, device=DEV)
    ops.ce_fwd_bwd(buf, 0, w, loss, smoothing=smoothing, labels=labels)
    check(loss[0], lref + 3.5, 1e-5, "ce loss, explicit labels, non-zero slot")
    _check_dlogits(buf, gref, w / rows, "ce dlogits, explicit labels")


def test_ce_out_of_range_labels():
    """labels = n and labels = -1 on one row each: the loss is NaN, the other rows' dlogits are what they would be, nothing
    beside the rows is touched (the logits are the middle rows of a larger buffer: no access can leave the allocation)"""
    rows, n, guard, w = 5, 65, 2, 0.25
    logits = 30 * torch.tanh(rnd(rows, n, seed=672, dtype=torch.float32))
    whole = torch.full((rows + 2 * guard, n), 77.0, device=DEV)
    whole[guard:guard + rows] = logits
    labels = torch.tensor([3, n, 10, -1, 64], device=DEV)
    loss = torch.zeros(1, device=DEV)
    ops.ce_fwd_bwd(whole[guard:guard + rows], 0, w, loss, labels=labels)
    assert bool(torch.isnan(loss[0]))
    good = torch.tensor([0, 2, 4], device=DEV)
    lg = logits[good].double().requires_grad_(True)
    (w / rows * F.cross_entropy(lg, labels[good], reduction="sum")).backward()
    got = whole[guard:guard + rows]
    assert torch.isfinite(got).all()
    _check_dlogits(got[good], lg.grad, w / rows, "ce dlogits beside an out-of-range row")
    assert bool((whole[:guard] == 77.0).all()) and bool((whole[guard + rows:] == 77.0).all())


@pytest.mark.parametrize("d", [8, 63, 64, 65, 512, 1000])
@pytest.mark.parametrize("rows", [1, 5, 130])
def test_l2norm_shapes(rows, d):
    """one wave per row strides d by 64, four rows per workgroup: d below / at / above a wave, rows = 130 ends in half a
    workgroup; against fp64"""
    a = rnd(rows, d, seed=680, dtype=torch.float32)
    ar = a.double().requires_grad_(True)
    yref = ar / ar.norm(dim=1, keepdim=True)
    y, nrm = ops.l2norm_fwd(a)
    check(y, yref.detach(), 1e-5, "l2norm")
    check(nrm, ar.detach().norm(dim=1), 1e-5, "l2norm norm")
    dy = rnd(rows, d, seed=681, dtype=torch.float32)
    yref.backward(dy.double())
    check(ops.l2norm_bwd(dy, y, nrm), ar.grad, 1e-4, "l2norm bwd")


def test_eos_all_zero_mask_row():
    """a row without any real token: sum(mask) - 1 = -1, which the reference uses as a Python index -- the LAST position
    [ref: model/clip.py:67-68]"""
    b, t, h = 3, 16, 64
    lens = torch.tensor([5, 0, 16], device=DEV)
    mask = (torch.arange(t, device=DEV)[None] < lens[:, None]).long()
    hid = rnd(b * t, h, seed=690)
    hv = hid.view(b, t, h)
    out = ops.eos_gather(hid, mask, b, t, h)
    assert torch.equal(out[1], hv[:, -1][1].float())
    assert torch.equal(out, hv[torch.arange(b, device=DEV), lens - 1].float())
    d = rnd(b, h, seed=691, dtype=torch.float32)
    want = torch.zeros(b, t, h, device=DEV, dtype=BF)
    want[torch.arange(b, device=DEV), lens - 1] = d.to(BF)
    assert torch.equal(ops.eos_scatter(d, mask, b, t, h).view(b, t, h), want)
