"""Tiny driver for PMC passes over the fused 5x5 depthwise backward (conv_lane.hip MODE 3 at K = 5, 24-channel tiles) and the two
launches it replaces: two launches of each per shape, 32 images (run under rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, one
counter per run).  Prints the algorithmic bytes of each launch: the fused one reads dd + e and writes dZ0."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import mammo_clip_amd  # noqa: F401
import mammo_clip_amd.lib as L
from mammo_clip_amd import ops

DEV = torch.device("cuda:0")
b, k, pad = 32, 5, 2
lib = L.load()
lib.mc_dwconv_set_lane_mode(1)
for c, h, w in ((384, 190, 114), (1056, 95, 57)):
    e = torch.randn(b * h * w, c, device=DEV).to(ops.BF16)
    dd = torch.randn(b * h * w, c, device=DEV).to(ops.BF16)
    wk = torch.randn(k * k, c, device=DEV)
    st = ops.BNStats()
    st.mean, st.invstd, st.scale, st.shift, st.count = (torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.ones(c, device=DEV),
                                                        torch.zeros(c, device=DEV), float(b * h * w))
    wflip = wk.flip(0).contiguous()
    for _ in range(2):
        ops.dwconv_bwd_data(dd, wk, b, h, w, c, k, 1, pad, pad, h, w, w_kkc_flipped=wflip, epi=(e, st))
        ops.dwconv_bwd_weight(e, dd, b, h, w, c, k, 1, pad, pad, h, w, pro=(st.scale, st.shift))
        ops.dwconv_bwd_fused(dd, e, st, wflip, b, h, w, c, k, pad, pad, h, w)
    torch.cuda.synchronize()
    t = 2 * c * b * h * w
    print(f"alg MB c={c}: data gradient read {2 * t / 1e6:.1f} write {t / 1e6:.1f}; weight gradient read {2 * t / 1e6:.1f}; fused read {2 * t / 1e6:.1f} write {t / 1e6:.1f}")
lib.mc_dwconv_set_lane_mode(-1)
