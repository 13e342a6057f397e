#!/usr/bin/env python3
"""Times the device-side training augmentation (mammo_clip_amd/augment.py, mc_augment_u8) at the workload's own shape:
64 output images of 1520 x 912 from 32 sources -- both views of 32 pairs -- with the reference's transform config
(alpha 10, sigma 15) and all four steps (both flips, affine, elastic) on in every row.

HIP events after a warm-up, REPS repeats, median / min / max.  The two kernels are timed on their own through the
mc_augment_set_stages developer switch (same launches, same data).  Bytes: what the op must move is one source read and the
three output planes (4 H W per image); the int16 intermediate (written once, read once plus halo: 8 H W) is listed apart.
The cost of two views is set against the training step's time per pair (--pair-ms: ms per pair of `python bench.py` on the
same box; default the README's 8.36 s / 1024 pairs).  Prints one JSON line.

    python scripts/augment_bench.py [--reps 10] [--pair-ms 8.164]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mammo_clip_amd import augment as A, lib as L, ops  # noqa: E402


def event_us(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return us


def stats(us, n_img):
    med = statistics.median(us)
    return {"median_us": round(med, 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "reps": len(us),
            "us_per_image": round(med / n_img, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sources", type=int, default=32)
    ap.add_argument("--height", type=int, default=1520)
    ap.add_argument("--width", type=int, default=912)
    ap.add_argument("--pair-ms", type=float, default=8360.0 / 1024, help="training step time per pair, ms")
    args = ap.parse_args()
    dev = torch.device("cuda")
    H, W, ns = args.height, args.width, args.sources
    n = 2 * ns
    gen = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, 256, (ns, H, W), device=dev, generator=gen, dtype=torch.uint8)
    pol = A.AugmentPolicy.from_transform_config({"affine_transform_degree": 20, "affine_translate_percent": 0.1,
                                                 "affine_scale": [0.8, 1.2], "affine_shear": 20, "elastic_transform_alpha": 10,
                                                 "elastic_transform_sigma": 15, "p": 1.0}, size=(H, W))
    d = pol.draw(n, torch.Generator().manual_seed(0))
    for k in ("hflip", "vflip", "affine", "elastic"):
        d[k][:] = True
    rows = pol.rows(d, H, W, np.arange(n) % ns)
    out = torch.empty((n, 3, H, W), dtype=torch.uint8, device=dev)
    lib = L.load()
    # Rows, taps and workspace are allocated per call by ops.augment_u8, as a training loop would; the upload of the few
    # integers is part of the timed call.
    call = lambda: ops.augment_u8(src, rows, pol.sigma, out=out)   # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "images": n, "sources": ns, "height": H, "width": W,
           "sigma": pol.sigma, "alpha": pol.alpha, "radius": int(4 * pol.sigma + 0.5)}
    try:
        res["augment"] = stats(event_us(call, args.reps), n)
        L.check(lib.mc_augment_set_stages(1))
        res["aug_hpass_k"] = stats(event_us(call, args.reps, warmup=1), n)
        L.check(lib.mc_augment_set_stages(2))
        res["aug_warp_k"] = stats(event_us(call, args.reps, warmup=1), n)
    finally:
        lib.mc_augment_set_stages(3)
    sec = res["augment"]["median_us"] * 1e-6
    res["gbps_source_and_output"] = round(n * 4.0 * H * W / sec / 1e9, 1)
    res["gbps_with_intermediate"] = round(n * 12.0 * H * W / sec / 1e9, 1)
    taps = 2 * res["radius"] + 1
    res["gmacs_per_s"] = round(n * 4.0 * taps * H * W / sec / 1e9, 1)           # 2 components x 2 passes x taps per pixel
    res["pair_ms"] = round(args.pair_ms, 4)
    res["two_views_share_of_pair_step"] = round(2 * res["augment"]["us_per_image"] * 1e-3 / args.pair_ms, 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
