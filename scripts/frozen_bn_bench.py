#!/usr/bin/env python3
"""Frozen BatchNorm (EfficientNet.freeze_bn / backward in eval mode), two measurements on the device:

  sites   the one-pass backward kernel (ops.bnact_bwd(frozen=True): mc_bnact_bwd_frozen + the frozen finalize) against the
          two-pass training-mode ops.bnact_bwd (reduce, finalize, apply) on the same tensors, at every distinct BatchNorm2 site
          (act 0, upstream gradient g, drop-connect row scale) and the head site (SiLU, pooled-mean gradient) of EfficientNet-B5
          on a micro-batch of 32 pairs at 1520 x 912 (32 images per encoder call).  HIP events after a warm-up around
          back-to-back calls of the ops wrapper (output allocation and finalize included; as many calls as give >= 3 ms of device
          work per window, 8 .. 256, from a first estimate),
          the two forms alternating, median of --reps windows, reported per call; GB/s = algorithmic bytes (two-pass: x and g read twice, dx written; one-pass: read
          once, dx written) over the median.
  step    Trainer.step of the cfg3 workload (B5, 32 pairs, 1520 x 912, T = 256, HIP AdamW) in train mode and with freeze_bn(),
          alternating, host clock around a step that ends in a device synchronise.

Prints one JSON line.

    python scripts/frozen_bn_bench.py [--reps 10] [--step-reps 3] [--skip-step] [--skip-sites]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mammo_clip_amd import engine, lib as L, ops  # noqa: E402
from mammo_clip_amd.breastclip.loss import build_loss  # noqa: E402
from mammo_clip_amd.breastclip.model import build_model  # noqa: E402
from mammo_clip_amd.breastclip.model.modules.efficientnet_custom import EfficientNet  # noqa: E402
from mammo_clip_amd.breastclip.optimizer import build_optimizer  # noqa: E402

N_IMG, H, W, T = 32, 1520, 912, 256
WINDOW_US = 3000.0        # device work per timed window: as many back-to-back calls as fill it (8 .. 256)


def site_shapes():
    """distinct (hw, c, act, kind) of the BatchNorm2 sites and the head of B5 at N_IMG x H x W"""
    enc = EfficientNet.from_name("efficientnet-b5")
    n, h, w = enc.stem_geo(N_IMG, H, W)
    out = []
    for blk in enc._blocks:
        n, h, w = blk.out_geo(n, h, w)
        s = (h * w, blk.args.cout, 0, "bn2")
        if s not in out:
            out.append(s)
    out.append((h * w, enc.out_dim, 1, "head"))
    return out


def time_pair(fa, fb, reps, lead, warmup=3):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()

    def window(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lead.fill_(0.0)                    # device work for the host to enqueue behind
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / inner

    inner = int(min(256, max(8, -(-WINDOW_US // min(window(fa, 8), window(fb, 8))))))
    ua, ub = [], []
    for _ in range(reps):
        for fn, us in ((fa, ua), (fb, ub)):
            us.append(window(fn, inner))
    return statistics.median(ua), statistics.median(ub), inner


def bench_sites(reps, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    lead = torch.empty(1 << 26, dtype=torch.float32, device=dev)
    rows = []
    for hw, c, act, kind in site_shapes():
        m = N_IMG * hw
        x = torch.randn(m, c, generator=gen, device=dev).to(ops.BF16)
        g = torch.randn(m, c, generator=gen, device=dev).to(ops.BF16) if kind == "bn2" else None
        gamma = torch.rand(c, generator=gen, device=dev) + 0.5
        beta = torch.randn(c, generator=gen, device=dev) * 0.1
        rm, rv = torch.randn(c, generator=gen, device=dev) * 0.1, torch.rand(c, generator=gen, device=dev) + 0.5
        st = ops.bn_eval_coeffs(gamma, beta, rm, rv, 1e-3)
        kw = dict(g=g, rowscale=torch.ones(N_IMG, device=dev)) if kind == "bn2" else \
            dict(add=torch.randn(N_IMG, c, generator=gen, device=dev), add_scale=1.0 / hw)
        two = lambda: ops.bnact_bwd(x, N_IMG, hw, c, st, gamma, act, **kw)                    # noqa: E731
        one = lambda: ops.bnact_bwd(x, N_IMG, hw, c, st, gamma, act, frozen=True, **kw)       # noqa: E731
        t2, t1, inner = time_pair(two, one, reps, lead)
        el = 2 * m * c
        reads = 2 if g is not None else 1
        rows.append({"site": kind, "hw": hw, "c": c, "calls_per_window": inner, "two_pass_us": round(t2, 1), "one_pass_us": round(t1, 1),
                     "ratio": round(t1 / t2, 3), "two_pass_gbps": round(el * (2 * reads + 1) / t2 / 1e3, 1),
                     "one_pass_gbps": round(el * (reads + 1) / t1 / 1e3, 1)})
        del x, g
    return rows


def bench_step(reps, dev):
    import bench as B
    enc_name = B.WORKLOADS["cfg3"][0]
    model = build_model(B.model_cfg(enc_name), B.LOSS_CFG, types.SimpleNamespace(vocab_size=28996)).to(dev)
    lossf = build_loss(B.LOSS_CFG)
    opt = build_optimizer(model, {"name": "adamw", "config": {"lr": 1e-6, "weight_decay": 1e-4}})
    tr = engine.Trainer(model, lossf, opt, None, dev)
    batch = B.synth_batch_gpu(N_IMG, H, W, T, dev, seed=0)
    times = {False: [], True: []}
    for rep in range(reps + 1):                       # (the first round is the warm-up of both modes)
        for frozen in (False, True):
            model.freeze_bn(frozen)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tr.step(batch)
            torch.cuda.synchronize()
            if rep:
                times[frozen].append(1e3 * (time.perf_counter() - t0))
            assert torch.isfinite(out["total"]).all()
    model.freeze_bn(False)
    return {"train_ms": round(statistics.median(times[False]), 1), "frozen_ms": round(statistics.median(times[True]), 1),
            "train_all_ms": [round(t, 1) for t in times[False]], "frozen_all_ms": [round(t, 1) for t in times[True]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-sites", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: timings are taken on the GPU only")
    dev = torch.device("cuda")
    L.load()
    res = {"device": torch.cuda.get_device_name(0), "storage": L.STORAGE, "images_per_call": N_IMG, "h": H, "w": W}
    if not args.skip_sites:
        res["sites"] = bench_sites(args.reps, dev)
    if not args.skip_step:
        res["cfg3_step"] = bench_step(args.step_reps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
