"""Every row of the exact-arithmetic depthwise tables (tests/_dwconv_exact_cases.py), without a device: the fp64 reference is
built and proves the conditions under which the kernels' arithmetic is exact, and the library's host-only plan queries
(mc_dwconv_march_plan, mc_dwconv_lane_plan, mc_dwconv_bwd_data_plan) confirm that the launch reaches the strip, segment, image
group, unit or tile seam the row names -- so a changed tile constant fails here instead of silently emptying
tests/test_dwconv_exact_gpu.py."""
import ctypes as C

import pytest

import _dwconv_exact_cases as X
from mammo_clip_amd import lib as L


@pytest.mark.parametrize("cs", X.CASES, ids=X.case_id)
def test_row_is_exact_and_reaches_its_seam(cs):
    X.check_exact(cs, X.ref_of(cs))
    p = X.route(cs)
    assert cs.kind == "gather" or p["rows"] >= 1, "the library does not take this argument block"
    X.check_route(cs, p)


def test_tables_cover_every_form():
    """both lane modes, both kernel sizes and strides, every kind plain and saturated where it exists, and every seam name"""
    have = {(cs.kind, cs.sat, cs.lane, cs.k, cs.s) for cs in X.CASES}
    for k in (3, 5):
        for s in (1, 2):
            for lane in (0, 1):
                for kind, sat in (("fwd", False), ("fwd", True), ("wgrad", False), ("wgrad", True)):
                    assert (kind, sat, lane, k, s) in have, (kind, sat, lane, k, s)
        for lane in (0, 1):
            assert ("dgrad1", True, lane, k, 1) in have
        assert ("fused", True, 1, k, 1) in have and ("gather", False, 0, k, 1) in have
        assert ("dgrad2", False, 0, k, 2) in have and ("dgrad2", True, 0, k, 2) in have
    seams = {cs.seam for cs in X.CASES}
    assert seams >= {"strip+1", "strip-mid", "segs2", "segs3", "strips2xsegs2", "ragged-wg", "s2-strips-segs", "group", "group-ragged",
                     "past-G4", "past-G2", "units-mid-image", "units-straddle", "xcd-contiguous", "ring", "tiles3", "tiles12w", "slot-fewer"}


def test_fallback_reference_of_the_saturated_cases():
    """the Gaussian reference the saturated rows fall back to (a device whose sigmoid does not saturate) builds, is finite and
    consistent with itself, and some row of every saturated kind is small enough for it"""
    import torch
    small = {cs.kind for cs in X.CASES if cs.sat and cs.n * X.geom(cs)[2] * X.geom(cs)[3] <= X.FALLBACK_MAX_PIXELS}
    assert small == {"fwd", "wgrad", "dgrad1", "dgrad2", "fused"}
    for cs in (X.CASES[0], next(c for c in X.CASES if c.s == 2 and c.k == 5)):
        pl, pt, oh, ow = X.geom(cs)
        r = X.reference_gauss(cs.k, cs.s, cs.n, cs.h, cs.w, cs.c)
        assert r.y.shape == (cs.n, oh, ow, cs.c) and r.dx_a0.shape == r.e.shape == r.dsilu.shape and r.dw.shape == r.dw_rounded.shape == r.wk.shape
        assert all(bool(torch.isfinite(t).all()) for t in r)
        # a0 rounded to the storage type moves dW by the rounding error of a0 at most
        assert float((r.dw - r.dw_rounded).abs().max()) <= 2.0 ** -8 * float((r.dy.abs().sum() / cs.c) * 4)
        z = r.e * r.scale + r.shift
        assert torch.allclose(r.dsilu, torch.sigmoid(z) * (1 + z * (1 - torch.sigmoid(z))))


def test_plan_queries_agree_with_the_row_counts_of_the_launches():
    """the plans' return values are the workspace rows the sizing queries promise under the matching lane mode, and argument
    blocks no form takes are answered with 0"""
    lib = L.load()
    old = lib.mc_dwconv_set_lane_mode(0)
    try:
        for cs in X.CASES:
            if cs.kind not in ("fwd", "wgrad", "dgrad1"):
                continue
            lib.mc_dwconv_set_lane_mode(cs.lane)
            a = X.dw_args(cs, "conv" if cs.kind != "dgrad1" else "flipped")
            if cs.kind == "dgrad1":
                a.epi_x = 16
            rows = lib.mc_dwconv_bwd_weight_dw_rows(C.byref(a)) if cs.kind == "wgrad" else lib.mc_dwconv_stat_rows(C.byref(a))
            assert rows == X.route(cs)["rows"], X.case_id(cs)
    finally:
        lib.mc_dwconv_set_lane_mode(old)
    fused = [cs for cs in X.CASES if cs.kind == "fused"]
    for cs in fused:
        a = X.dw_args(cs, "flipped")
        a.epi_x = 16
        assert lib.mc_dwconv_bwd_fused_stat_rows(C.byref(a)) == lib.mc_dwconv_bwd_fused_dw_rows(C.byref(a)) == X.route(cs)["rows"]
    a, plan = X.dw_args(fused[0], "flipped"), (C.c_int * 8)()
    assert lib.mc_dwconv_lane_plan(C.byref(a), 4, plan) == 0 and lib.mc_dwconv_lane_plan(C.byref(a), -1, plan) == 0
    a.stride = 2
    assert lib.mc_dwconv_lane_plan(C.byref(a), 1, plan) == 0 and lib.mc_dwconv_lane_plan(C.byref(a), 3, plan) == 0
    a.k = 4
    assert lib.mc_dwconv_lane_plan(C.byref(a), 0, plan) == 0 and lib.mc_dwconv_march_plan(C.byref(a), 0, plan) == 0
