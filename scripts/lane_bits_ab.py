#!/usr/bin/env python3
"""Bit-level A/B of two builds of the depthwise kernels (conv_lane.hip and the marching kernels of conv.hip; developer tool).
The fused forward (MODE 4), the fused backward with its e rows formed from the block input (MODE 5) and the weight gradients
have no bit-exact reference inside the tree, so a change that must not move results is checked against the build before it:

  python scripts/lane_bits_ab.py --dump DIR        outputs of all six lane modes (m0 .. m5), for whatever library is loaded, as
                                                   .npy files (16-bit tensors as int16 images, statistics partials and dW as
                                                   float32), and of the marching form (lane mode 0): a0 / a1 / a2 = forward with
                                                   prologue and statistics, stride-1 data gradient with the epilogue, weight
                                                   gradient over the lane cases; s2 / s2e / s2x = stride-2 data gradient plain,
                                                   with the epilogue, and formed from the block input with dw_out
  python scripts/lane_bits_ab.py --compare A B     two such directories: 16-bit tensors must be identical; float tensors are
                                                   reported as identical / identical up to the sign of zero / max difference
                                                   relative to the tensor's largest magnitude.  The marching form's statistics
                                                   partials (one workgroup's sum in a fixed order per row) must be identical
                                                   too; dW (atomic sums across workgroups) is reported per tensor kind.

Run the dump once per library (scripts/ab_libs.sh, or copy the library to compare over mammo_clip_amd/lib/libmammoclip_hip.so
in between).  The shapes are the lane / fused / xdw cases of tests/test_kernels_gpu.py, the stride-2 epilogue cases there and
the cases of tests/test_dw_s2_efree_gpu.py."""
import os
import sys

import numpy as np

LANE_CASES = [  # k, s, n, h, w, c
    (5, 1, 3, 150, 260, 96), (5, 1, 5, 95, 57, 72), (5, 1, 2, 61, 130, 40), (3, 1, 2, 70, 300, 48), (3, 1, 3, 33, 59, 24),
    (5, 2, 2, 120, 250, 48), (3, 2, 3, 77, 131, 40), (5, 1, 33, 48, 29, 32), (5, 1, 1, 300, 114, 64), (5, 1, 70, 1100, 40, 32),
    (5, 1, 5, 6, 5, 40), (3, 1, 9, 7, 9, 24), (5, 2, 3, 9, 11, 16)]
FUSED_CASES = [  # n, h, w, c
    (2, 70, 300, 48), (3, 33, 59, 24), (5, 95, 57, 72), (33, 48, 29, 64), (9, 7, 9, 24), (2, 40, 33, 240), (1, 200, 62, 40),
    (70, 600, 40, 32)]
XDW_CASES = [  # k, s, n, h, w, cin, c
    (3, 1, 2, 70, 300, 40, 240), (3, 2, 2, 77, 131, 24, 144), (5, 2, 2, 120, 250, 40, 240), (5, 1, 3, 150, 130, 64, 384),
    (3, 2, 3, 61, 95, 64, 384), (3, 1, 5, 95, 57, 128, 768), (5, 1, 3, 48, 57, 128, 200), (5, 1, 9, 48, 29, 48, 288),
    (3, 1, 9, 7, 9, 16, 96), (5, 2, 3, 9, 11, 24, 144), (5, 1, 2, 33, 70, 88, 528), (3, 1, 1, 20, 20, 8, 48)]
XE_CASES = [  # n, h, w, cin, c
    (2, 70, 300, 40, 240), (3, 33, 59, 24, 144), (5, 95, 57, 64, 72), (33, 48, 29, 16, 96), (9, 7, 9, 8, 24), (1, 200, 62, 48, 40),
    (2, 41, 130, 64, 384)]
S2_CASES = [  # k, n, h, w, c, (pad_l, pad_t): test_dwconv_s2_dgrad_with_bn_backward_epilogue
    (3, 2, 40, 33, 144, (0, 1)), (3, 2, 41, 34, 240, (1, 1)), (5, 2, 29, 23, 384, (1, 2)), (5, 1, 60, 64, 64, (2, 2)),
    (3, 3, 17, 50, 48, (0, 0)), (5, 2, 30, 31, 1056, (2, 1))]
S2X_CASES = [  # n, h, w, cin, c, (pad_l, pad_t): tests/test_dw_s2_efree_gpu.py::CASES
    (2, 40, 33, 24, 144, (0, 1)), (2, 41, 34, 40, 240, (1, 1)), (3, 17, 50, 8, 48, (0, 1)), (1, 3, 3, 16, 24, (1, 1)),
    (5, 38, 22, 64, 384, (0, 1)), (2, 9, 300, 24, 144, (0, 1)), (1, 140, 12, 32, 72, (1, 1)), (17, 6, 7, 48, 40, (0, 1))]


def dump(out_dir):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import mammo_clip_amd  # noqa: F401
    import mammo_clip_amd.lib as L
    from mammo_clip_amd import ops

    dev = torch.device("cuda:0")
    lib = L.load()
    os.makedirs(out_dir, exist_ok=True)

    def rnd(*shape, seed=0, scale=1.0, dtype=None):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(*shape, generator=g) * scale).to(dev).to(ops.BF16 if dtype is None else dtype)

    def save(name, t):
        t = t.contiguous()
        a = t.view(torch.int16).cpu().numpy() if t.dtype != torch.float32 else t.cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)

    def stats_of(e, c, rows, seed):
        gamma, beta = rnd(c, seed=seed, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=seed + 1, dtype=torch.float32) * 0.1
        ef = e.float()
        mean, var = ef.mean(0), ef.var(0, unbiased=False)
        st = ops.BNStats()
        st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
        st.scale = (gamma * st.invstd).contiguous()
        st.shift = (beta - mean * st.scale).contiguous()
        st.count = float(rows)
        return st

    old = lib.mc_dwconv_set_lane_mode(1)                # the lane = column form wherever it is supported
    try:
        for i, (k, s, n, h, w, c) in enumerate(LANE_CASES):
            pad = (k - 1) // 2 if s == 1 else (k - 2) // 2
            oh, ow = (h + s - 1) // s, (w + s - 1) // s
            x, dy = rnd(n * h * w, c, seed=31), rnd(n * oh * ow, c, seed=42)
            wk = rnd(k * k, c, seed=32, dtype=torch.float32) * 0.3
            pro = (rnd(c, seed=33, dtype=torch.float32) * 0.3 + 1.0, rnd(c, seed=34, dtype=torch.float32) * 0.3)
            y, part = ops.dwconv_fwd(x, wk, n, h, w, c, k, s, pad, pad, oh, ow, pro=pro, stats=True)
            save(f"m0_{i}_y", y)
            save(f"m0_{i}_part", part)
            save(f"m2_{i}_dw", ops.dwconv_bwd_weight(x, dy, n, h, w, c, k, s, pad, pad, oh, ow, pro=pro))
            if s == 1:
                st = stats_of(x, c, n * h * w, 4)
                dz, part = ops.dwconv_bwd_data(dy, wk, n, h, w, c, k, 1, pad, pad, h, w, w_kkc_flipped=wk.flip(0).contiguous(), epi=(x, st))
                save(f"m1_{i}_dz", dz)
                save(f"m1_{i}_part", part)
            del x, dy, y
        for i, (n, h, w, c) in enumerate(FUSED_CASES):
            e, dd = rnd(n * h * w, c, seed=1), rnd(n * h * w, c, seed=2)
            wk = rnd(9, c, seed=3, dtype=torch.float32)
            st = stats_of(e, c, n * h * w, 4)
            dz, part, dw = ops.dwconv_bwd_fused(dd, e, st, wk.flip(0).contiguous(), n, h, w, c, 3, 1, 1, h, w)
            save(f"m3_{i}_dz", dz)
            save(f"m3_{i}_part", part)
            save(f"m3_{i}_dw", dw)
            del e, dd, dz
        for i, (k, s, n, h, w, cin, c) in enumerate(XDW_CASES):
            pad = (k - 1) // 2 if s == 1 else (k - 2) // 2
            oh, ow = (h + s - 1) // s, (w + s - 1) // s
            x, we = rnd(n * h * w, cin, seed=41), rnd(c, cin, seed=42, scale=cin ** -0.5)
            wk = rnd(k * k, c, seed=43, dtype=torch.float32) * 0.3
            pro = (rnd(c, seed=44, dtype=torch.float32) * 0.3 + 1.0, rnd(c, seed=45, dtype=torch.float32) * 0.3)
            y, part = ops.mbconv_xdw_fwd(x, we, pro, wk, n, h, w, c, k, s, pad, pad, oh, ow, stats=True)
            save(f"m4_{i}_y", y)
            save(f"m4_{i}_part", part)
        for i, (n, h, w, cin, c) in enumerate(XE_CASES):
            x, we = rnd(n * h * w, cin, seed=71), rnd(c, cin, seed=72, scale=cin ** -0.5)
            dd = rnd(n * h * w, c, seed=73)
            wk = rnd(9, c, seed=74, dtype=torch.float32)
            st = stats_of(ops.linear_fwd(x, we), c, n * h * w, 75)
            dz, part, dw = ops.dwconv_bwd_fused(dd, None, st, wk.flip(0).contiguous(), n, h, w, c, 3, 1, 1, h, w, xw=(x, we))
            save(f"m5_{i}_dz", dz)
            save(f"m5_{i}_part", part)
            save(f"m5_{i}_dw", dw)
        lib.mc_dwconv_set_lane_mode(0)                  # the marching form
        for i, (k, s, n, h, w, c) in enumerate(LANE_CASES):
            pad = (k - 1) // 2 if s == 1 else (k - 2) // 2
            oh, ow = (h + s - 1) // s, (w + s - 1) // s
            x, dy = rnd(n * h * w, c, seed=31), rnd(n * oh * ow, c, seed=42)
            wk = rnd(k * k, c, seed=32, dtype=torch.float32) * 0.3
            pro = (rnd(c, seed=33, dtype=torch.float32) * 0.3 + 1.0, rnd(c, seed=34, dtype=torch.float32) * 0.3)
            y, part = ops.dwconv_fwd(x, wk, n, h, w, c, k, s, pad, pad, oh, ow, pro=pro, stats=True)
            save(f"a0_{i}_y", y)
            save(f"a0_{i}_part", part)
            save(f"a2_{i}_dw", ops.dwconv_bwd_weight(x, dy, n, h, w, c, k, s, pad, pad, oh, ow, pro=pro))
            if s == 1:
                st = stats_of(x, c, n * h * w, 4)
                dz, part = ops.dwconv_bwd_data(dy, wk, n, h, w, c, k, 1, pad, pad, h, w, w_kkc_flipped=wk.flip(0).contiguous(), epi=(x, st))
                save(f"a1_{i}_dz", dz)
                save(f"a1_{i}_part", part)
            del x, dy, y
        for i, (k, n, h, w, c, (pl, pt)) in enumerate(S2_CASES):
            oh, ow = (h + 1) // 2, (w + 1) // 2
            e, dd = rnd(n * h * w, c, seed=1), rnd(n * oh * ow, c, seed=2)
            wk = rnd(k * k, c, seed=3, dtype=torch.float32)
            st = stats_of(e, c, n * h * w, 4)
            save(f"s2_{i}_dx", ops.dwconv_bwd_data(dd, wk, n, h, w, c, k, 2, pl, pt, oh, ow))
            dz, part = ops.dwconv_bwd_data(dd, wk, n, h, w, c, k, 2, pl, pt, oh, ow, epi=(e, st))
            save(f"s2e_{i}_dz", dz)
            save(f"s2e_{i}_part", part)
        for i, (n, h, w, cin, c, (pl, pt)) in enumerate(S2X_CASES):
            oh, ow = (h + 1) // 2, (w + 1) // 2
            x, we = rnd(n * h * w, cin, seed=81), rnd(c, cin, seed=82, scale=cin ** -0.5)
            dd = rnd(n * oh * ow, c, seed=83)
            wk = rnd(9, c, seed=84, dtype=torch.float32)
            st = stats_of(ops.linear_fwd(x, we), c, n * h * w, 85)
            save(f"s2_x{i}_dx", ops.dwconv_bwd_data(dd, wk, n, h, w, c, 3, 2, pl, pt, oh, ow))
            dz, part, dw = ops.dwconv_bwd_data(dd, wk, n, h, w, c, 3, 2, pl, pt, oh, ow, epi=(None, st), xw=(x, we), dw=True)
            save(f"s2x_{i}_dz", dz)
            save(f"s2x_{i}_part", part)
            save(f"s2x_{i}_dw", dw)
    finally:
        lib.mc_dwconv_set_lane_mode(old)
    torch.cuda.synchronize()
    print(f"dumped {len(os.listdir(out_dir))} tensors to {out_dir} [{L.STORAGE} storage]")


def compare(a_dir, b_dir):
    names = sorted(os.listdir(a_dir))
    assert names == sorted(os.listdir(b_dir)), "the two dumps hold different tensors"
    bad16, badpart, worst = 0, 0, {}
    counts = {"identical": 0, "identical up to the sign of zero": 0, "different": 0}
    for nm in names:
        a, b = np.load(os.path.join(a_dir, nm)), np.load(os.path.join(b_dir, nm))
        assert a.shape == b.shape, nm
        if a.dtype == np.int16:
            if not np.array_equal(a, b):
                bad16 += 1
                print(f"16-bit tensor {nm}: {int((a != b).sum())} of {a.size} elements differ")
            continue
        kind = nm.split("_")[0] + ("_dw" if nm.endswith("_dw.npy") else "_part")
        if np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            counts["identical"] += 1
        elif np.array_equal(a, b):                      # +0 == -0
            counts["identical up to the sign of zero"] += 1
            if kind.endswith("_part") and kind[0] in "as":
                badpart += 1
                print(f"statistics partials {nm} differ in the sign of a zero")
        else:
            counts["different"] += 1
            assert np.isfinite(a).all() and np.isfinite(b).all(), nm
            rel = float(np.abs(a.astype(np.float64) - b).max() / np.abs(a).max())
            worst[kind] = max(worst.get(kind, 0.0), rel)
            if kind.endswith("_part") and kind[0] in "as":      # marching form: a workgroup's sum in a fixed order
                badpart += 1
                print(f"statistics partials {nm} differ: {rel:.2e} of the largest magnitude")
    n16 = sum(1 for nm in names if np.load(os.path.join(a_dir, nm), mmap_mode="r").dtype == np.int16)
    print(f"16-bit output tensors: {n16 - bad16} of {n16} identical")
    print("float tensors (statistics partials, dW): " + ", ".join(f"{v} {k}" for k, v in counts.items()))
    for kind, rel in sorted(worst.items()):
        print(f"  largest difference / largest magnitude, {kind}: {rel:.2e}")
    return 0 if bad16 == 0 and badpart == 0 else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
