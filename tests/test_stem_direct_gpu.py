"""Direct stem convolution (csrc/stem.hip: mc_stem_conv_fwd / _fwd_u8 / _wgrad) against the path it replaces, mc_stem_im2col +
the row-streaming GEMMs, on the same inputs.  GPU only (`pytest -m gpu`).

The kernels work on tiles of SR = 4 output rows x TW = 64 output pixels (one wave per row, four 16-pixel fragments per wave),
persistent workgroups: at most 1024 (forward) / 768 (weight gradient) / 512 (weight gradient with the BatchNorm0 apply) of them
walk the tiles.  Shapes are the smallest that reach
every seam:
  * ow = 63 / 64 / 65 (one below, equal to, one above a strip) and 129 (three strips), oh = 1 / 4 / 5 (one row, a full tile, one
    row above it), n = 1 and 3;
  * even and odd h / w under the (0, 1, 0, 1) padding of an even nominal size: the right / bottom padding row is read (even) or
    not (odd); (1, 1, 1, 1), the padding of an odd nominal size, for left / top padding (the scalar load path);
  * every stem width the kernels are instantiated for (c0 = 32, 40, 48, 56, 64);
  * one case of 1122 tiles (2 x 264 x 2050): more tiles than workgroups in both launches, so workgroups take a second tile;
  * fp32 and raw uint8 sources; a channels-first tensor takes the im2col path (module level).
Checks:
  * forward: torch.equal to stem_im2col + linear_fwd on the row-streaming kernel (both feed the same bf16 operands to ONE K = 32
    step of the same MFMA);
  * statistics: column sums and the finalized BatchNorm coefficients within the 1e-4 of max|ref| the GEMM statistics tests use
    (tests/test_kernels_gpu.py: "rows colsum", "bn affine");
  * weight gradient: fp64 de^T . patches from the 16-bit operands, within 2e-3 of max|ref| -- the bound of
    tests/test_kernels_gpu.py::test_gemm_wgrad_tn, whose cases include (999, 48, 32); columns 27..31 exactly zero; two calls
    give the same bits (fixed-order sums, no atomics);
  * BatchNorm0 apply inside the weight gradient (bn = (e, coef)): the same comparison with de = coef[0]*dZ0 + coef[1]*e + coef[2]
    formed in fp64 from the same coefficients and rounded to 16 bits; the existing bnact_bwd + linear_wgrad sequence is printed
    beside it;
  * module: _StemFn + block 0 of B2 at n = 2, 34 x 22 with MC_STEM_DIRECT off and on (MC_STEM_FOLD_BN0 off and on), train mode,
    StatTape record then replay: outputs bit-equal, parameter gradients within the 2e-3 above.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
import mammo_clip_amd.lib as L  # noqa: E402
from mammo_clip_amd import ops  # noqa: E402
from mammo_clip_amd.breastclip.model.modules import efficientnet_custom as encmod  # noqa: E402
from oracle import arch as oarch, weights as ow  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16
TW, SR = 64, 4
P0, P1 = (0, 1, 0, 1), (1, 1, 1, 1)
#        n  h    w     pad c0
CASES = [(1, 2, 126, P0, 48), (3, 3, 127, P0, 48), (1, 8, 128, P0, 48), (3, 9, 129, P0, 32), (1, 10, 130, P0, 40),
         (3, 11, 258, P0, 48), (2, 9, 129, P1, 48), (1, 8, 128, P1, 56), (1, 3, 126, P0, 64), (2, 264, 2050, P0, 48)]
IDS = [f"n{n}-{h}x{w}-pad{p[0]}{p[2]}-c{c}" for n, h, w, p, c in CASES]


def out_extent(size, lo, hi):
    return (size + lo + hi - 3) // 2 + 1


def relerr(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-300))


def test_cases_reach_every_seam():
    geo = [(n, out_extent(h, p[2], p[3]), out_extent(w, p[0], p[1])) for n, h, w, p, _ in CASES]
    assert {n for n, _, _ in geo} >= {1, 3}
    assert {ow for _, _, ow in geo} >= {TW - 1, TW, TW + 1, 2 * TW + 1}
    assert {oh for _, oh, _ in geo} >= {1, SR, SR + 1}
    assert {c for *_, c in CASES} == {32, 40, 48, 56, 64}
    lib = L.load()
    n, oh, ow = geo[-1]
    assert [lib.mc_stem_conv_blocks(n, oh, ow, k) for k in (1, 0, 2)] == [1024, 768, 512]      # tiles > workgroups
    assert lib.mc_stem_conv_blocks(*geo[0], 1) == 1


@functools.lru_cache(maxsize=None)
def case(i, src):
    """inputs and the reference results of case i (computed once, shared by the tests)"""
    n, h, w, pad, c0 = CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    if src == "u8":
        x = ops.RawImages(torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(DEV).permute(0, 3, 1, 2), 0.3, 0.2)
    else:
        x = torch.randn(n, h, w, 3, generator=g).to(DEV).permute(0, 3, 1, 2)          # the trainer's permuted view
    wt = (torch.randn(c0, 3, 3, 3, generator=g) * 27 ** -0.5).to(DEV)
    l, r, t, b = pad
    oh, ow = out_extent(h, t, b), out_extent(w, l, r)
    de = torch.randn(n * oh * ow, c0, generator=g).to(DEV).to(BF)
    wb = ops.stem_weight_prep(wt)
    patches = ops.stem_im2col(x, l, t, oh, ow)
    prev = ops.set_rows_select_scale(1 << 20)          # the row-streaming kernels at any row count: the kernels of the workload
    try:
        e_ref, part_ref = ops.linear_fwd(patches, wb, stats=True)
        dw_ref_kernel = ops.linear_wgrad(de, patches)
    finally:
        ops.set_rows_select_scale(prev)
    dw64 = de.double().T @ patches.double()
    torch.cuda.synchronize()
    return dict(x=x, wb=wb, de=de, geo=(n, oh, ow, l, t, c0), e_ref=e_ref, part_ref=part_ref, dw64=dw64, dw_ref_kernel=dw_ref_kernel,
                patches=patches)


@pytest.mark.parametrize("src", ["fp32", "u8"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward_and_statistics(i, src):
    d = case(i, src)
    n, oh, ow, l, t, c0 = d["geo"]
    assert ops.stem_direct_ok(d["x"], c0, l, t)
    e, part = ops.stem_conv_fwd(d["x"], d["wb"], l, t, oh, ow, stats=True)
    e_plain = ops.stem_conv_fwd(d["x"], d["wb"], l, t, oh, ow)
    assert torch.equal(e, d["e_ref"]), f"max |diff| {float((e.float() - d['e_ref'].float()).abs().max())}"
    assert torch.equal(e_plain, e)
    assert part.shape == (L.load().mc_stem_conv_blocks(n, oh, ow, 1), 2, c0)
    ef = e.double()
    got, ref = part.double().sum(0), d["part_ref"].double().sum(0)
    for k, (what, exact) in enumerate([("colsum", ef.sum(0)), ("colsumsq", (ef * ef).sum(0))]):
        print(f"{what}: vs fp64 {relerr(got[k], exact):.2e}, reference kernel vs fp64 {relerr(ref[k], exact):.2e}")
        assert relerr(got[k], exact) <= 1e-4, what
    gamma, beta = torch.linspace(0.5, 1.5, c0, device=DEV), torch.linspace(-0.2, 0.2, c0, device=DEV)
    st = ops.bn_finalize(part, n * oh * ow, gamma, beta, None, None, 0.01, 1e-3, False)
    st_ref = ops.bn_finalize(d["part_ref"], n * oh * ow, gamma, beta, None, None, 0.01, 1e-3, False)
    for what in ("scale", "shift", "mean", "invstd"):
        err = relerr(getattr(st, what), getattr(st_ref, what))
        print(f"finalized {what}: {err:.2e}")
        assert err <= 1e-4, what


@pytest.mark.parametrize("src", ["fp32", "u8"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_weight_gradient(i, src):
    d = case(i, src)
    n, oh, ow, l, t, c0 = d["geo"]
    dw = ops.stem_conv_wgrad(d["de"], d["x"], l, t, oh, ow)
    assert dw.shape == (c0, 32) and torch.isfinite(dw).all()
    print(f"dw vs fp64: {relerr(dw, d['dw64']):.2e} (linear_wgrad: {relerr(d['dw_ref_kernel'], d['dw64']):.2e})")
    assert relerr(dw, d["dw64"]) <= 2e-3
    assert torch.equal(dw[:, 27:], torch.zeros_like(dw[:, 27:]))
    assert torch.equal(ops.stem_conv_wgrad(d["de"], d["x"], l, t, oh, ow), dw)        # fixed-order sums: the same bits


@pytest.mark.parametrize("src", ["fp32", "u8"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_weight_gradient_with_bn0_apply(i, src):
    """de is dZ0; the coefficients are those of the BatchNorm0 backward of e with dZ0's own reductions (ops.bn_bwd_coefs)"""
    d = case(i, src)
    n, oh, ow, l, t, c0 = d["geo"]
    e, dz, count = d["e_ref"], d["de"], n * oh * ow
    gamma, beta = torch.linspace(0.5, 1.5, c0, device=DEV), torch.linspace(-0.2, 0.2, c0, device=DEV)
    st = ops.bn_finalize(d["part_ref"], count, gamma, beta, None, None, 0.01, 1e-3, False)
    xhat = (e.float() - st.mean) * st.invstd
    part = torch.stack([dz.float().sum(0), (dz.float() * xhat).sum(0)])[None].contiguous()
    coef, _, _ = ops.bn_bwd_coefs(part, count, st, gamma)
    dw = ops.stem_conv_wgrad(dz, d["x"], l, t, oh, ow, bn=(e, coef))
    k = coef.double()
    de64 = (k[0] * dz.double() + k[1] * e.double() + k[2]).to(BF).double()
    ref = de64.T @ d["patches"].double()
    de_seq, _, _ = ops.bnact_bwd(e, n, oh * ow, c0, st, gamma, 0, g=dz, partials=part)
    prev = ops.set_rows_select_scale(1 << 20)
    try:
        dw_seq = ops.linear_wgrad(de_seq, d["patches"])
    finally:
        ops.set_rows_select_scale(prev)
    print(f"dw (bn0 apply inside) vs fp64: {relerr(dw, ref):.2e} (bnact_bwd + linear_wgrad: {relerr(dw_seq, ref):.2e})")
    assert dw.shape == (c0, 32) and torch.isfinite(dw).all()
    assert relerr(dw, ref) <= 2e-3
    assert torch.equal(dw[:, 27:], torch.zeros_like(dw[:, 27:]))
    assert torch.equal(ops.stem_conv_wgrad(dz, d["x"], l, t, oh, ow, bn=(e, coef)), dw)


# ------------------------------------------------------------------------------------------------ module level
@functools.lru_cache(maxsize=None)
def _encoder():
    arch = oarch.build_arch("efficientnet-b2")
    enc = encmod.EfficientNet.from_name("efficientnet-b2")
    enc.load_state_dict(ow.synth_state_dict(ow.efficientnet_shapes(arch), seed=10), strict=True)
    return enc.to(DEV)


def _stem_block0(enc, x, direct, fold=True):
    """train-mode stem + block 0: record forward (no graph), replay forward with a graph, backward -> (outputs, gradients)"""
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    old = encmod.STEM_DIRECT, encmod.STEM_FOLD_BN0
    encmod.STEM_DIRECT, encmod.STEM_FOLD_BN0 = direct, fold
    try:
        enc.train()
        enc.zero_grad(set_to_none=True)
        tape = encmod.StatTape()

        def fwd():
            call = encmod._Call(tape)
            y, link, (n, h, w) = enc._stem(x, call)
            return enc._blocks[0](y, n, h, w, None, link, call)
        with torch.no_grad():
            y_rec = fwd()
        tape.replay()
        y = fwd()
        r = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
        (y.float() * r).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    finally:
        encmod.STEM_DIRECT, encmod.STEM_FOLD_BN0 = old
        enc.load_state_dict(state)
    return (y_rec, y.detach()), grads


@pytest.mark.parametrize("src", ["fp32", "u8"])
def test_stem_fn_direct_matches_im2col(src):
    enc = _encoder()
    n, h, w = 2, 34, 22
    g = torch.Generator().manual_seed(7)
    if src == "u8":
        x = ops.RawImages(torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(DEV).permute(0, 3, 1, 2), 0.3, 0.2)
        x_cf = ops.RawImages(x.data.contiguous(), 0.3, 0.2)
    else:
        x = torch.randn(n, h, w, 3, generator=g).to(DEV).permute(0, 3, 1, 2)
        x_cf = x.contiguous()
    c0 = enc._conv_stem.weight.shape[0]
    l, _, t, _ = enc.stem_pad
    assert ops.stem_direct_ok(x, c0, l, t) and not ops.stem_direct_ok(x_cf, c0, l, t)
    ys0, g0 = _stem_block0(enc, x, False)
    ys1, g1 = _stem_block0(enc, x, True, fold=False)
    ys2, g2 = _stem_block0(enc, x, True, fold=True)
    ysc, gc = _stem_block0(enc, x_cf, True)                # channels-first: the im2col path whatever the switch says
    assert torch.equal(ys0[0], ys0[1])
    for ys in (ys1, ys2, ysc):
        assert torch.equal(ys[0], ys0[0]) and torch.equal(ys[1], ys0[1])
    assert "_conv_stem.weight" in g0 and g0.keys() == g1.keys() == g2.keys() == gc.keys()
    for k in g0:
        assert torch.equal(gc[k], g0[k]), k
        for gd in (g1, g2):
            err = relerr(gd[k], g0[k])
            assert err <= 2e-3, (k, err)
    print("stem weight gradient vs im2col: direct", relerr(g1["_conv_stem.weight"], g0["_conv_stem.weight"]),
          "direct + bn0 apply inside", relerr(g2["_conv_stem.weight"], g0["_conv_stem.weight"]))
