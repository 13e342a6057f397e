"""Host side of the fused 5x5 stride-1 depthwise backward (no device needed): the predicates of its own through which the 12-wave
instances of mc_dwconv_bwd_fused are asked for, and the blocks of EfficientNet-B5 / -B2 whose plan takes them.  The predicates of
the 3x3 instances keep their answers (tests/test_host_cpu.py pins those, 5x5 shapes included)."""
import ctypes as C

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import lib as L


def dw(c, k, s, h, w, n=32, epi=True):
    a = L.DwconvArgs()
    a.n, a.h, a.w, a.c, a.k, a.stride, a.pad_l, a.pad_t, a.oh, a.ow = n, h, w, c, k, s, (k - 1) // 2, (k - 1) // 2, h, w
    a.epi_x = 16 if epi else None
    return a


def test_fused5_predicates():
    lib = L.load()
    sup = lambda a: bool(lib.mc_dwconv_bwd_fused5_supported(C.byref(a)))      # noqa: E731
    pref = lambda a: bool(lib.mc_dwconv_bwd_fused5_preferred(C.byref(a)))     # noqa: E731
    # the four measured shapes of B5 at 1520 x 912 (profiles/lane5_fused_ab.md)
    for c, h, w in ((384, 190, 114), (768, 95, 57), (1056, 95, 57), (1824, 48, 29)):
        assert sup(dw(c, 5, 1, h, w)) and pref(dw(c, 5, 1, h, w)), (c, h, w)
        assert not lib.mc_dwconv_bwd_fused_supported(C.byref(dw(c, 5, 1, h, w)))       # the 3x3 predicate keeps its answer
    # supported, not measured: narrow tensors, 30-49 column maps, one image on a narrow map
    for a in (dw(240, 5, 1, 190, 114), dw(1056, 5, 1, 60, 40), dw(1824, 5, 1, 48, 29, n=1)):
        assert sup(a) and not pref(a)
    assert sup(dw(40, 5, 1, 9, 29)) and sup(dw(8, 5, 1, 3, 130))                     # ragged and single 24-channel tiles
    # not 5x5, not stride 1, no epilogue operands, channels not a multiple of 8, e rows from the block input
    assert not sup(dw(768, 3, 1, 95, 57)) and not sup(dw(240, 5, 2, 380, 228)) and not sup(dw(384, 5, 1, 190, 114, epi=False))
    assert not sup(dw(380, 5, 1, 190, 114))
    a = dw(384, 5, 1, 190, 114)
    a.xw, a.cin = 16, 64
    assert not sup(a)
    # the sizing helpers are common to both kernel sizes
    a = dw(384, 5, 1, 190, 114)
    assert lib.mc_dwconv_bwd_fused_dw_rows(C.byref(a)) == lib.mc_dwconv_bwd_fused_stat_rows(C.byref(a)) >= 2


def test_plans_take_the_fused_5x5_backward():
    """fused_dw5 per block at the per-GPU batch of the timed workloads; fused_dw (the 3x3 launch) never set beside it"""
    from mammo_clip_amd.breastclip.model.modules.efficientnet_custom import EfficientNet
    want = {("efficientnet-b5", 32, 1520, 912): list(range(9, 13)) + list(range(20, 27)) + list(range(28, 36)),
            ("efficientnet-b2", 64, 912, 912): list(range(12, 16)) + list(range(17, 21))}
    for (name, n, H, W), blocks in want.items():
        enc = EfficientNet.from_name(name).train()
        for recording in (True, False):
            geo, got = enc.stem_geo(n, H, W), []
            for blk in enc._blocks:
                p = blk.plan(*geo, recording)
                assert not (p.fused_dw and p.fused_dw5)
                assert not p.fused_dw5 or (blk.args.k == 5 and blk.args.s == 1)
                if p.fused_dw5:
                    got.append(blk.args.idx)
                geo = blk.out_geo(*geo)
            assert got == (blocks if recording else []), (name, recording, got)
