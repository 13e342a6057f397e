"""Developer timing of the backward of the stride-2 3x3 depthwise blocks with a narrow input (B5 blocks 3 and 13, 32 images):
the three launches that rebuild and read the expanded tensor e (expand GEMM, weight gradient with the BatchNorm0 + swish
prologue, data gradient with the BatchNorm-backward epilogue) against the one launch that forms its e rows from the block input
(mc_dwconv_bwd_data with xw + dw_out), alternating old / new / old / new in one process.
usage: python scripts/dw_s2_efree_ab.py [once]      (once: one launch of the new form at block 3's shape, for a counter pass)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import ops

DEV = torch.device("cuda:0")
n, k = 32, 3
SHAPES = ((24, 144, 760, 456, (0, 0)), (64, 384, 190, 114, (0, 0)))      # cin, c, h, w, (pad_l, pad_t)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


once = len(sys.argv) > 1 and sys.argv[1] == "once"
for (cin, c, h, w, (pl, pt)) in SHAPES[:1] if once else SHAPES:
    oh, ow = (h + 1) // 2, (w + 1) // 2
    x = torch.randn(n * h * w, cin, device=DEV).to(ops.BF16)
    we = (torch.randn(c, cin, device=DEV) * cin ** -0.5).to(ops.BF16)
    dd = torch.randn(n * oh * ow, c, device=DEV).to(ops.BF16)
    wk = torch.randn(k * k, c, device=DEV)
    st = ops.BNStats()
    st.mean, st.invstd = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    st.scale, st.shift, st.count = torch.ones(c, device=DEV), torch.zeros(c, device=DEV), float(n * h * w)
    geo = (n, h, w, c, k, 2, pl, pt, oh, ow)
    new = lambda: ops.dwconv_bwd_data(dd, wk, *geo, epi=(None, st), xw=(x, we), dw=True)
    if once:
        new()
        torch.cuda.synchronize()
        floor = 2.0 * n * (c * (oh * ow + h * w) + cin * h * w)
        print(f"one launch of the E-free form, {cin}->{c} {h}x{w}: algorithmic bytes dD + x + dZ0 = {floor / 1e9:.3f} GB")
        break
    e = ops.linear_fwd(x, we)
    olds = (("rebuild e (expand GEMM)", lambda: ops.linear_fwd(x, we)),
            ("weight gradient (e, dD)", lambda: ops.dwconv_bwd_weight(e, dd, *geo, pro=(st.scale, st.shift))),
            ("data gradient + bn0 epilogue (e, dD)", lambda: ops.dwconv_bwd_data(dd, wk, *geo, epi=(e, st))))
    print(f"block {cin}->{c} {h}x{w}, {n} images, prefers the new launch: {ops.dwconv_bwd_s2_xw_ok(*geo, cin=cin)}")
    for rep in range(2):
        t_old = [timed(fn) for _, fn in olds]
        t_new = timed(new)
        for (nm, _), t in zip(olds, t_old):
            print(f"  repeat {rep}  old  {nm:40s} {t:8.1f} us")
        by = 2.0 * n * (c * (oh * ow + h * w) + cin * h * w)
        print(f"  repeat {rep}  old  sum {sum(t_old):8.1f} us   new (one launch, e rows from x) {t_new:8.1f} us   {by / t_new / 1e3:7.1f} GB/s of dD + x + dZ0"
              f"   ratio {sum(t_old) / t_new:.2f}")
    del e, x, dd
