"""Host predicates of the E-free stride-2 depthwise backward (mc_dwconv_bwd_data with xw): pure functions of the argument block,
no device needed."""
import ctypes as C

from mammo_clip_amd import lib as L


def _dw(cin, c, k, s, h, w, n=32, epi=True, xw=True):
    a = L.DwconvArgs()
    a.n, a.h, a.w, a.c, a.k, a.stride, a.pad_l, a.pad_t, a.oh, a.ow = n, h, w, c, k, s, 0, 0, (h + 1) // 2, (w + 1) // 2
    a.epi_x = 16 if epi else None
    a.xw, a.cin = (16 if xw else None), cin
    return a


def test_s2_xw_predicates_and_plan():
    lib = L.load()
    sup = lambda a: bool(lib.mc_dwconv_bwd_data_xw_supported(C.byref(a)))
    pref = lambda a: bool(lib.mc_dwconv_bwd_data_xw_preferred(C.byref(a)))
    # B5 blocks 3 and 13 at 32 images of 1520 x 912: the measured shapes
    assert sup(_dw(24, 144, 3, 2, 760, 456)) and pref(_dw(24, 144, 3, 2, 760, 456))
    assert sup(_dw(64, 384, 3, 2, 190, 114)) and pref(_dw(64, 384, 3, 2, 190, 114))
    # small maps: supported, not preferred (not measured)
    assert sup(_dw(24, 144, 3, 2, 40, 34, n=2)) and not pref(_dw(24, 144, 3, 2, 40, 34, n=2))
    # 5x5, stride 1, wide or ragged inputs, missing operands: not taken
    assert not sup(_dw(40, 240, 5, 2, 380, 228)) and not sup(_dw(40, 240, 3, 1, 380, 228))
    assert not sup(_dw(128, 768, 3, 2, 96, 58)) and not sup(_dw(20, 120, 3, 2, 96, 58))
    assert not sup(_dw(24, 144, 3, 2, 760, 456, epi=False)) and not sup(_dw(24, 144, 3, 2, 760, 456, xw=False))
    assert not pref(_dw(128, 768, 3, 2, 96, 58))
    # the work split is the e-reading launch's: same partial rows with and without xw
    plan = (C.c_int * 4)()
    for a in (_dw(24, 144, 3, 2, 760, 456), _dw(64, 384, 3, 2, 190, 114), _dw(32, 72, 3, 2, 140, 12, n=1)):
        rows = lib.mc_dwconv_bwd_data_plan(C.byref(a), plan)
        b = _dw(a.cin, a.c, 3, 2, a.h, a.w, n=a.n, xw=False)
        assert rows == lib.mc_dwconv_bwd_data_stat_rows(C.byref(a)) == lib.mc_dwconv_bwd_data_stat_rows(C.byref(b)) > 0
        assert plan[0] >= 1 and plan[1] >= 1 and plan[2] % 4 == 0 and plan[3] == -(-a.c // (48 if a.c % 48 == 0 and a.c < 192 else 64))
