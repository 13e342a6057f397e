"""The E-free backward of the stride-2 3x3 depthwise conv: mc_dwconv_bwd_data with xw forms the e rows of the pixels it completes
from the block input x and the expand weight on the MFMA unit (instead of reading the expanded tensor) and, with dw_out, is the
conv's weight gradient too [ref: efficientnet_custom.py:104-111 backwards].  GPU only (`pytest -m gpu`).  Every bound below is the
one tests/test_kernels_gpu.py / tests/test_fullsize_gpu.py already use for the same comparison."""
import ctypes as C
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16
GUARD = 4096                  # elements of NaN in front of and behind every 16-bit operand (a multiple of 8: 16-byte alignment)


def rnd(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def relerr(got, ref):
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def banded(t):
    """the same values in the middle of a NaN-filled allocation: whatever a launch reads in front of or behind the tensor is a NaN"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=DEV, dtype=t.dtype)
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


def bn_stats(e, c, rows, seed):
    gamma, beta = rnd(c, seed=seed, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=seed + 1, dtype=torch.float32) * 0.1
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(rows)
    return st, gamma


def out_hw(h, w):
    return (h + 1) // 2, (w + 1) // 2


def plan_of(n, h, w, c, pad):
    """(strips, segments, super-rows per segment, channel tiles) of the launch, from the library's own plan function"""
    oh, ow = out_hw(h, w)
    a = ops._dw_args(n, h, w, c, 3, 2, pad[0], pad[1], oh, ow)
    a.epi_x = 16
    plan = (C.c_int * 4)()
    rows = L.load().mc_dwconv_bwd_data_plan(C.byref(a), plan)
    assert rows == L.load().mc_dwconv_bwd_data_stat_rows(C.byref(a)) > 0
    return tuple(plan)


def operands(n, h, w, cin, c):
    """the generator of test_dwconv_fused_backward_with_e_rows_formed_from_the_block_input, dd on the stride-2 output geometry"""
    oh, ow = out_hw(h, w)
    x = rnd(n * h * w, cin, seed=71)
    we = rnd(c, cin, seed=72, scale=cin ** -0.5)
    dd = rnd(n * oh * ow, c, seed=73)
    wk = rnd(9, c, seed=74, dtype=torch.float32)
    e = ops.linear_fwd(x, we)                                  # the stored tensor
    st, gamma = bn_stats(e, c, n * h * w, 75)
    return x, we, dd, wk, e, st, gamma


def reference(dd, wk, e, st, n, h, w, c, pad):
    """the launches the new one replaces, on the GEMM's stored e"""
    oh, ow = out_hw(h, w)
    dz, part = ops.dwconv_bwd_data(dd, wk, n, h, w, c, 3, 2, pad[0], pad[1], oh, ow, epi=(e, st))
    dw = ops.dwconv_bwd_weight(e, dd, n, h, w, c, 3, 2, pad[0], pad[1], oh, ow, pro=(st.scale, st.shift))
    return dz, part, dw


def efree(dd, wk, x, we, st, n, h, w, c, pad, dw=True):
    oh, ow = out_hw(h, w)
    return ops.dwconv_bwd_data(dd, wk, n, h, w, c, 3, 2, pad[0], pad[1], oh, ow, epi=(None, st), xw=(x, we), dw=dw)


def partial_err(part_ref, part):
    s0, s1 = part_ref.double().sum(0), part.double().sum(0)
    scale = s0.abs().amax(dim=1, keepdim=True)
    return float(((s0 - s1).abs() / scale).max())


def compare(n, h, w, cin, c, pad, what=""):
    """Test 1's comparison and bounds; returns the measured figures"""
    x, we, dd, wk, e, st, _ = operands(n, h, w, cin, c)
    oh, ow = out_hw(h, w)
    assert ops.dwconv_bwd_s2_xw_ok(n, h, w, c, 3, 2, pad[0], pad[1], oh, ow, cin=cin, force=True)
    dz_ref, part_ref, dw_ref = reference(dd, wk, e, st, n, h, w, c, pad)
    for _ in range(2):                                         # twice: a stale accumulator would show
        dz, part, dw = efree(dd, wk, x, we, st, n, h, w, c, pad)
    torch.cuda.synchronize()
    assert part.shape == part_ref.shape
    assert torch.isfinite(dz.float()).all() and torch.isfinite(part).all() and torch.isfinite(dw).all(), what
    fig = dict(dz=relerr(dz, dz_ref), equal=float((dz == dz_ref).float().mean()), part=partial_err(part_ref, part),
               dw=float((dw - dw_ref).abs().max()) / float(dw_ref.abs().max()))
    print(what, (n, h, w, cin, c, pad), fig)
    assert fig["dz"] <= 1e-2, (what, fig)
    assert fig["equal"] >= 0.98, (what, fig)                   # almost every element bit-identical: the staged e IS the stored e
    assert fig["part"] <= 2e-3, (what, fig)
    assert fig["dw"] <= 2e-3, (what, fig)
    return fig


# n, h, w, cin, c, (pad_l, pad_t)
CASES = [
    (2, 40, 33, 24, 144, (0, 1)),
    (2, 41, 34, 40, 240, (1, 1)),
    (3, 17, 50, 8, 48, (0, 1)),
    (1, 3, 3, 16, 24, (1, 1)),
    (5, 38, 22, 64, 384, (0, 1)),       # two k-steps
    (2, 9, 300, 24, 144, (0, 1)),       # more than one strip
    (1, 140, 12, 32, 72, (1, 1)),       # more than one row segment; ragged channel tile
    (17, 6, 7, 48, 40, (0, 1)),         # image count above the item grouping
]


@pytest.mark.parametrize("n,h,w,cin,c,pad", CASES)
def test_s2_data_gradient_with_e_rows_formed_from_the_block_input(n, h, w, cin, c, pad):
    """mc_dwconv_bwd_data with xw + dw_out against the two launches it replaces (the e-reading data gradient and the weight
    gradient with the BatchNorm0 + swish prologue) on e = the expand GEMM's stored output: the staged e is the same fp32
    accumulation rounded once to 16 bits, so dZ0, the partials and dW agree to the last-bit spread of two MFMA accumulation
    orders."""
    strips, segs, seg_rows, ctiles = plan_of(n, h, w, c, pad)
    if (h, w) == (9, 300):
        assert strips > 1, strips
    if (h, w) == (140, 12):
        assert segs > 1 and (c % ctiles != 0 or c // ctiles not in (48, 64)), (segs, ctiles)     # (tiles hold 48 or 64 channels)
    compare(n, h, w, cin, c, pad)


@pytest.mark.parametrize("n,h,w,cin,c,pad", [CASES[0], CASES[1], CASES[4], CASES[6]])
def test_s2_exact_e_equals_the_e_reading_launch(n, h, w, cin, c, pad):
    """The expand weight is a 0/1 selection matrix, so the staged e IS x[:, sel] exactly and dZ0 must equal the e-reading launch
    on e = x[:, sel] BIT FOR BIT; partials and dW finite and within Test 1's bounds.  Before the launches under test one launch
    runs on operands that are NaN everywhere (dy tile, e tiles: every LDS slot a launch can reach then holds NaN patterns when
    the next launch starts on that CU); x, e and dd sit between NaN guard bands in memory."""
    oh, ow = out_hw(h, w)
    x = banded(rnd(n * h * w, cin, seed=71))
    sel = torch.arange(c, device=DEV) * 7 % cin                 # asymmetric: expanded channel i reads input channel 7 i mod cin
    we = torch.zeros(c, cin, device=DEV)
    we[torch.arange(c, device=DEV), sel] = 1.0
    we = we.to(BF)
    e = banded(x[:, sel].contiguous())
    dd = banded(rnd(n * oh * ow, c, seed=73))
    wk = rnd(9, c, seed=74, dtype=torch.float32)
    st, _ = bn_stats(e, c, n * h * w, 75)
    dz_ref, part_ref, dw_ref = reference(dd, wk, e, st, n, h, w, c, pad)
    efree(torch.full_like(dd, float("nan")), wk, torch.full_like(x, float("nan")), we, st, n, h, w, c, pad)
    for _ in range(2):
        dz, part, dw = efree(dd, wk, x, we, st, n, h, w, c, pad)
    dz_only, part_only = efree(dd, wk, x, we, st, n, h, w, c, pad, dw=False)      # (the form without the weight gradient)
    torch.cuda.synchronize()
    assert torch.equal(dz, dz_ref), "dZ0 (e rows from x) differs from the e-reading launch"
    assert torch.equal(dz_only, dz) and torch.equal(part_only, part)
    assert torch.isfinite(part).all() and torch.isfinite(dw).all()
    assert partial_err(part_ref, part) <= 2e-3, "BatchNorm-backward partials"
    assert float((dw - dw_ref).abs().max()) <= 2e-3 * float(dw_ref.abs().max()), "dW"


@pytest.mark.parametrize("n,h,w,cin,c,pad", [CASES[0], CASES[4]])
def test_s2_efree_chain_against_fp32_autograd(n, h, w, cin, c, pad):
    """x -> e = x We^T -> bn0 (the given batch statistics) -> silu -> depthwise 3x3 stride 2 in fp32 torch with autograd, on the
    same 16-bit operands: dZ0 within 1.5e-2, dgamma / dbeta (through bnact_bwd on the launch's partials) within 1e-2 -- the
    tolerances of test_dwconv_s2_dgrad_with_bn_backward_epilogue."""
    import torch.nn.functional as F
    x, we, dd, wk, e, st, gamma = operands(n, h, w, cin, c)
    oh, ow = out_hw(h, w)
    pl, pt = pad
    pr, pb = (ow - 1) * 2 + 3 - w - pl, (oh - 1) * 2 + 3 - h - pt
    ef = x.float() @ we.float().T
    z = (ef * st.scale + st.shift).requires_grad_(True)
    a0 = (z * torch.sigmoid(z)).view(n, h, w, c).permute(0, 3, 1, 2)
    y = F.conv2d(F.pad(a0, (pl, pr, pt, pb)), wk.t().reshape(c, 1, 3, 3), stride=2, groups=c)
    assert y.shape == (n, c, oh, ow)
    (y * dd.float().view(n, oh, ow, c).permute(0, 3, 1, 2)).sum().backward()
    dz_ref = z.grad
    xhat = (ef - st.mean) * st.invstd
    dz, part, dw = efree(dd, wk, x, we, st, n, h, w, c, pad)
    _, dg, db = ops.bnact_bwd(e, n, h * w, c, st, gamma, 0, g=dz, partials=part)
    torch.cuda.synchronize()
    fig = dict(dz=relerr(dz, dz_ref), dgamma=relerr(dg, (dz_ref * xhat).sum(0)), dbeta=relerr(db, dz_ref.sum(0)))
    print("vs fp32 autograd", (n, h, w, cin, c, pad), fig)
    assert torch.isfinite(dz.float()).all()
    assert fig["dz"] <= 1.5e-2 and fig["dgamma"] <= 1e-2 and fig["dbeta"] <= 1e-2, fig


def _cos_flat(a, b):
    a, b = a.detach().float().reshape(-1).cpu().double(), b.detach().float().reshape(-1).cpu().double()
    return float((a @ b) / (a.norm() * b.norm() + 1e-300))


def test_block_backward_without_the_expanded_tensor():
    """One MBConvBlock with B5 block 3's geometry scaled down (24 -> 144, 3x3, stride 2, pad (0,1,0,1), 2 images of 40 x 34) in
    recompute mode 1 with the folded BatchNorm0 backward: the E-free backward against the one that rebuilds e.  Forward
    bit-identical (it does not change), e neither stored nor rebuilt, dx and every parameter gradient cosine >= 0.995 and norm
    within 3.5 % (the bounds of test_folded_bn0_backward_at_production_threshold_b5)."""
    from mammo_clip_amd.breastclip.model.modules import efficientnet_custom as encmod
    gp = encmod.GlobalParams(1.0, 1.0, 224, 0.2, 1, 0.99, 1e-3, 0.2, 8, None, True)
    n, h, w = 2, 40, 34
    torch.manual_seed(5)
    blk = encmod.MBConvBlock(encmod.BlockArgs(1, 3, 2, 6, 24, 40, 0.25, True), gp, (h, w)).to(DEV)
    assert blk.args.pad == (0, 1, 0, 1)
    with torch.no_grad():
        for nm, p_ in blk.named_parameters():
            if nm.endswith("_bn0.weight") or nm.endswith("_bn1.weight") or nm.endswith("_bn2.weight"):
                p_.copy_(1.0 + 0.2 * torch.randn_like(p_))
            elif nm.endswith(".bias"):
                p_.copy_(0.1 * torch.randn_like(p_))
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    blk.train()
    blk.recompute = 1
    x0 = rnd(n * h * w, 24, seed=11)
    oh, ow = blk.out_geo(n, h, w)[1:]
    r = rnd(n * oh * ow, 40, seed=12)
    old = (encmod.BN_FOLD_MIN_BYTES, encmod.BN_FOLD_S2_MIN_BYTES, ops.EFREE_S2, ops.XDW, encmod._expand_conv)
    res, rebuilds = {}, {0: 0, 2: 0}
    try:
        encmod.BN_FOLD_MIN_BYTES, encmod.BN_FOLD_S2_MIN_BYTES, ops.XDW = 0, 0, 1
        for arm in (0, 2):                                      # off / wherever the launch is supported (the map is small)
            ops.EFREE_S2 = arm

            def counted(*a_, _arm=arm, **kw):
                rebuilds[_arm] += 1
                return old[4](*a_, **kw)
            encmod._expand_conv = counted
            blk.load_state_dict(sd, strict=True)
            blk.zero_grad(set_to_none=True)
            xin = x0.clone().requires_grad_(True)
            y = blk(xin, n, h, w)
            node = y.grad_fn
            assert node.plan.efree_s2 == (arm == 2) and node.plan.fold_bn0 and node.plan.xdw and not node.plan.efree
            assert node.saved["e"] is None and not node.saved["efree"]
            calls0 = rebuilds[arm]
            y.backward(r)
            torch.cuda.synchronize()
            assert rebuilds[arm] - calls0 == (0 if arm == 2 else 1), rebuilds      # no rebuild GEMM in the E-free backward
            res[arm] = (y.detach().clone(), xin.grad.detach().clone(), {k: p_.grad.detach().clone() for k, p_ in blk.named_parameters()})
    finally:
        encmod.BN_FOLD_MIN_BYTES, encmod.BN_FOLD_S2_MIN_BYTES, ops.EFREE_S2, ops.XDW, encmod._expand_conv = old
    assert torch.equal(res[0][0], res[2][0])
    grads = dict(res[0][2], dx=res[0][1])
    new = dict(res[2][2], dx=res[2][1])
    worst = {}
    for k_ in grads:
        worst[k_] = (_cos_flat(new[k_], grads[k_]), float(new[k_].norm() / (grads[k_].norm() + 1e-30)))
    print("E-free stride-2 block backward vs rebuilt e:", worst)
    for k_, (cs, nr) in worst.items():
        assert cs >= 0.995 and 0.965 <= nr <= 1.035, (k_, cs, nr)


def test_s2_efree_random_geometry_screen():
    """40 seeded random geometries (3x3, stride 2, both static paddings per axis, 1-9 images, maps 3x3 to 60x200, cin 8-64, c 8-384)
    against the e-reading launches, with Test 1's bounds"""
    rng = random.Random(20)
    for i in range(40):
        n, h, w = rng.randint(1, 9), rng.randint(3, 60), rng.randint(3, 200)
        while n * h * w > 40000:                               # (keeps every case well under a second)
            n = max(1, n // 2)
            h = max(3, h * 2 // 3)
        cin, c = 8 * rng.randint(1, 8), 8 * rng.randint(1, 48)
        pad = (rng.randint(0, 1), rng.randint(0, 1))
        compare(n, h, w, cin, c, pad, what=f"fuzz {i}")
