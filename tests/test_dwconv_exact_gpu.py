"""The depthwise kernels of conv.hip (marching forms, lane mode 0) and conv_lane.hip (lane = column forms MODE 0-3, lane mode 1)
against an INDEPENDENT fp64 reference at their strip, row-segment, image-group, unit-range and channel-tile seams, on operands
for which the arithmetic is exact.  GPU only (`pytest -m gpu`).

Method (tests/_dwconv_exact_cases.py holds the tables, the references and the derivation).  Operands from {-1, +1}, taps from
{+-1, +-2, +-3}: outputs, BatchNorm statistics, BatchNorm-backward partials and weight gradients are exact integers whatever the
summation order, the reference is fp64 conv2d / autograd on the same integers and every comparison is torch.equal -- one output
row lost at a seam moves a sum by an odd integer, which no share-of-the-largest-output bound would notice.  The BN+SiLU prologue,
the BatchNorm-backward epilogue and the fused backward run saturated (scale 1, shift 19: silu(z) = z and silu'(z) = 1 exactly for
z in {18, 20}); test_sigmoid_saturates_exactly proves that on the device through the elementwise kernels of bnact.hip, which
share sigmoid_f / silu_grad_f with the kernels under test.  If it fails, the saturated cases fall back to Gaussian operands, an
fp64 reference and the bounds of test_kernels_gpu.py (1e-2 outputs, 4e-3 dW, 2e-4 of the column scale for partials) on the shapes
of at most 4096 output pixels.

Every launch goes through the C ABI on guarded buffers: 16-bit inputs in the middle of NaN-filled allocations; outputs, statistics
and dw_partials workspaces prefilled with a NaN bit pattern between guard elements that must come back bit-identical; workspaces
of exactly the rows the library's query promised, finite afterwards; dW accumulated into a seeded integer prefill.  Each case runs
twice on fresh buffers, the weight gradients with the atomic and with the store-and-sum ending.  The route of every row (strips,
segments, images per wave, units, tiles) is asserted through mc_dwconv_march_plan / mc_dwconv_lane_plan / mc_dwconv_bwd_data_plan
before the launch (and, without a device, for the whole table in tests/test_dwconv_exact_routes.py).  Because the reference is
independent, a failing row names the kernel at fault; the lane-equals-marching tests elsewhere stay as they are."""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402

import _dwconv_exact_cases as X  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16
F32, F64 = torch.float32, torch.float64
GUARD = 4096                  # guard elements in front of and behind every buffer (a multiple of 8: 16-byte alignment)
assert BF == X.ST


class Buf:
    """`shape` elements of `dtype` in the middle of an allocation of NaN bit patterns (0x7F81 / 0x7FC12345): an input holds `fill`
    and whatever a launch reads beside it is a NaN; an output keeps the pattern until the launch writes it; check() demands the
    GUARD elements in front and behind bit-identical."""

    def __init__(self, shape, dtype, fill=None):
        two = dtype != F32
        self.sent = 0x7F81 if two else 0x7FC12345
        numel = math.prod(shape)
        self.raw = torch.full((numel + 2 * GUARD,), self.sent, dtype=torch.int16 if two else torch.int32, device=DEV)
        self.t = self.raw.view(dtype)[GUARD:GUARD + numel].view(shape)
        assert self.t.data_ptr() % 16 == 0 and bool(torch.isnan(self.t).all())
        if fill is not None:
            self.t.copy_(fill.to(DEV).reshape(shape))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        assert bool((self.raw[:GUARD] == self.sent).all()) and bool((self.raw[-GUARD:] == self.sent).all()), f"{what}: a guard element changed"


def f32(t):
    return t.to(DEV).float().contiguous()


@functools.lru_cache(maxsize=1)
def saturates():
    """sigmoid_f on the device at z in {18, 20}: BN+SiLU of +-1 with scale 1, shift 19 through the elementwise kernels of bnact.hip
    (not under test) returns exactly {18, 20}, and their backward passes the gradient through unchanged"""
    c, rows = 16, 64
    g = torch.Generator().manual_seed(5)
    x = (torch.randint(0, 2, (rows, c), generator=g) * 2 - 1).to(DEV).to(BF)
    gr = (torch.randint(0, 2, (rows, c), generator=g) * 2 - 1).to(DEV).to(BF)
    st = ops.BNStats()
    st.scale, st.shift = torch.ones(c, device=DEV), torch.full((c,), X.SHIFT, device=DEV)
    st.mean, st.invstd, st.count = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), float(rows)
    a0 = ops.bnact_apply(x, 1, rows, c, st.scale, st.shift, 1)
    dz, part = ops.bnact_bwd_reduce_dz(x, 1, rows, c, st, 1, gr)
    torch.cuda.synchronize()
    s = part.double().sum(0)
    want = torch.stack([gr.double().sum(0), (gr.double() * x.double()).sum(0)])
    return bool(torch.equal(a0.double(), x.double() + X.SHIFT) and torch.equal(dz, gr) and torch.equal(s, want))


def test_sigmoid_saturates_exactly():
    """the precondition of every saturated case.  If this fails, they run their fallback (module docstring)."""
    assert saturates()


def operands(cs, exact):
    """(e, dy, wk, BatchNorm (scale, shift, mean, invstd), expected y, expected dZ0 / dx, expected dW) as fp64 on the CPU"""
    c = cs.c
    if exact:
        r = X.ref_of(cs)
        bn = (torch.ones(c), torch.full((c,), X.SHIFT), torch.zeros(c), torch.ones(c))
        return r.e, r.dy, r.wk, bn, r.y, r.dx, r.dw
    r = X.reference_gauss(cs.k, cs.s, cs.n, cs.h, cs.w, cs.c)
    return r.e, r.dy, r.wk, (r.scale, r.shift, r.mean, r.invstd), r.y, r.dx_a0 * r.dsilu, (r.dw if cs.kind == "fused" else r.dw_rounded)


def same(got, ref, exact, tol, what):
    ref = ref.to(DEV).reshape(got.shape)
    if exact:
        bad = (got.double() != ref).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}: {float(got[tuple(bad[0])])} != {float(ref[tuple(bad[0])])}"
    else:
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        print(what, "relative error", err)
        assert err <= tol, (what, err)


def same_sums(part, ref_rows, exact, what):
    """part [rows, 2, c] finite in every row; its rows summed = ref_rows [2, c] (None: that sum is not exact, not compared)"""
    assert bool(torch.isfinite(part).all()), f"{what}: a partials element was not written"
    s = part.double().sum(0)
    for i, ref in enumerate(ref_rows):
        if ref is None:
            continue
        ref = ref.to(DEV)
        if exact:
            assert torch.equal(s[i], ref), f"{what}: sum {i} differs in channels {(s[i] != ref).nonzero().flatten().tolist()[:8]}: {(s[i] - ref)[(s[i] != ref)][:8].tolist()}"
        else:
            err = float(((s[i] - ref).abs() / ref.abs().max()).max())
            print(what, "sum", i, "relative error", err)
            assert err <= X.TOL_PART, (what, i, err)


def launch(cs, exact, det, p):
    """one launch of the case on fresh buffers, compared with the reference"""
    lib = L.load()
    k, s, n, h, w, c = cs.k, cs.s, cs.n, cs.h, cs.w, cs.c
    pl, pt, oh, ow = X.geom(cs)
    e, dy, wk, bn, y_ref, dz_ref, dw_ref = operands(cs, exact)
    what = X.case_id(cs) + (" store-and-sum" if det else "")
    e16, dy16 = Buf((n * h * w, c), BF, e), Buf((n * oh * ow, c), BF, dy)
    st = ops.BNStats()
    st.scale, st.shift, st.mean, st.invstd = (f32(t) for t in bn)
    st.count = float(n * h * w)
    g = torch.Generator().manual_seed(11)
    pre = torch.randint(-8, 9, (k * k, c), generator=g).double()
    bufs = [e16, dy16]
    if cs.kind in ("fwd", "wgrad", "gather", "dgrad2"):
        a = ops._dw_args(n, h, w, c, k, s, pl, pt, oh, ow)
        wt = f32(wk)
        a.w_kkc = wt.data_ptr()
        if cs.sat and cs.kind in ("fwd", "wgrad"):
            a.pro_scale, a.pro_shift = st.scale.data_ptr(), st.shift.data_ptr()
    else:
        wt = f32(wk.flip(0))
        a = ops._dw_fused_args(dy16.t, wt, n, h, w, c, k, pl, pt, oh, ow, e16.t, st)
    if cs.kind == "fwd":
        out = Buf((n * oh * ow, c), BF)
        rows = lib.mc_dwconv_stat_rows(C.byref(a))
        assert rows == p["rows"] >= 1
        part = Buf((rows, 2, c), F32)
        a.x, a.out, a.stat_partials, a.stat_rows = e16.ptr, out.ptr, part.ptr, rows
        L.call("mc_dwconv_fwd", C.byref(a), ops._st())
        torch.cuda.synchronize()
        same(out.t, y_ref, exact, X.TOL_OUT, what + " y")
        ok = X.check_exact(cs, X.ref_of(cs)) if exact else (True, True)
        yy = out.t.double().cpu() if not exact else y_ref.reshape(-1, c)      # (not exact: the sums of the STORED output)
        same_sums(part.t, [yy.sum(0) if ok[0] else None, (yy * yy).sum(0) if ok[1] else None], exact, what)
        bufs += [out, part]
    elif cs.kind == "wgrad":
        dw = Buf((k * k, c), F32, pre)
        a.x, a.dy, a.out = e16.ptr, dy16.ptr, dw.ptr
        drows = lib.mc_dwconv_bwd_weight_dw_rows(C.byref(a))
        assert drows == p["rows"] >= 1
        bufs.append(dw)
        if det:
            ws = Buf((drows, k * k, c), F32)
            a.dw_partials, a.dw_rows = ws.ptr, drows
            bufs.append(ws)
        L.call("mc_dwconv_bwd_weight", C.byref(a), ops._st())
        torch.cuda.synchronize()
        assert not det or bool(torch.isfinite(ws.t).all()), f"{what}: a dw_partials element was not written"
        same(dw.t if exact else dw.t - pre.to(DEV), pre + dw_ref if exact else dw_ref, exact, X.TOL_DW, what + " dW")
    elif cs.kind in ("gather", "dgrad2"):
        out = Buf((n * h * w, c), BF)
        a.dy, a.out = dy16.ptr, out.ptr
        bufs.append(out)
        if cs.sat:
            a.epi_x, a.epi_scale, a.epi_shift = e16.ptr, st.scale.data_ptr(), st.shift.data_ptr()
            a.epi_mean, a.epi_invstd = st.mean.data_ptr(), st.invstd.data_ptr()
            rows = lib.mc_dwconv_bwd_data_stat_rows(C.byref(a))
            assert rows == p["rows"] >= 1
            part = Buf((rows, 2, c), F32)
            a.stat_partials, a.stat_rows = part.ptr, rows
            bufs.append(part)
        L.call("mc_dwconv_bwd_data", C.byref(a), ops._st())
        torch.cuda.synchronize()
        same(out.t, dz_ref, exact, X.TOL_OUT, what + " dx")
        if cs.sat:
            dz = dz_ref.reshape(-1, c) if exact else out.t.double().cpu()
            same_sums(part.t, [dz.sum(0), (dz * (e.reshape(-1, c) - bn[2]) * bn[3]).sum(0)], exact, what)
    else:                                              # dgrad1 (mc_dwconv_fwd on flipped taps with the epilogue) and fused
        out = Buf((n * h * w, c), BF)
        fused = cs.kind == "fused"
        rows = lib.mc_dwconv_bwd_fused_stat_rows(C.byref(a)) if fused else lib.mc_dwconv_stat_rows(C.byref(a))
        assert rows == p["rows"] >= 1
        part = Buf((rows, 2, c), F32)
        a.out, a.stat_partials, a.stat_rows = out.ptr, part.ptr, rows
        bufs += [out, part]
        if fused:
            dw = Buf((k * k, c), F32, pre)
            a.dw_out = dw.ptr
            bufs.append(dw)
            if det:
                drows = lib.mc_dwconv_bwd_fused_dw_rows(C.byref(a))
                assert drows == rows
                ws = Buf((drows, k * k, c), F32)
                a.dw_partials, a.dw_rows = ws.ptr, drows
                bufs.append(ws)
        L.call("mc_dwconv_bwd_fused" if fused else "mc_dwconv_fwd", C.byref(a), ops._st())
        torch.cuda.synchronize()
        same(out.t, dz_ref, exact, X.TOL_OUT, what + " dZ0")
        dz = dz_ref.reshape(-1, c) if exact else out.t.double().cpu()
        same_sums(part.t, [dz.sum(0), (dz * (e.reshape(-1, c) - bn[2]) * bn[3]).sum(0)], exact, what)
        if fused:
            assert not det or bool(torch.isfinite(ws.t).all()), f"{what}: a dw_partials element was not written"
            same(dw.t if exact else dw.t - pre.to(DEV), pre + dw_ref if exact else dw_ref, exact, X.TOL_DW, what + " dW")
    for b in bufs:
        b.check(what)
    assert bool(torch.equal(e16.t.double().cpu(), e.reshape(-1, c))) and bool(torch.equal(dy16.t.double().cpu(), dy.reshape(-1, c))), f"{what}: an input changed"


@pytest.mark.parametrize("cs", X.CASES, ids=X.case_id)
def test_dwconv_exact(cs):
    exact = not cs.sat or saturates()
    pl, pt, oh, ow = X.geom(cs)
    if not exact and cs.n * oh * ow > X.FALLBACK_MAX_PIXELS:
        pytest.skip("the fallback of the saturated cases runs the shapes of at most 4096 output pixels")
    if exact:
        X.check_exact(cs, X.ref_of(cs))
    lib = L.load()
    old = lib.mc_dwconv_set_lane_mode(cs.lane)
    try:
        p = X.route(cs)
        X.check_route(cs, p)
        for det in ((False, True) if cs.kind in ("wgrad", "fused") else (False,)):
            for _ in range(2):
                launch(cs, exact, det, p)
    finally:
        lib.mc_dwconv_set_lane_mode(old)
