#!/usr/bin/env python3
"""Times the weight EMA of the optimizer step (optim.hip: mc_adamw_step_ema, mc_ema_update) against the plain AdamW pass on
the real parameter list of the flagship model, EfficientNet-B5 + BioClinicalBERT (138 M fp32 parameters in ~700 tensors),
with synthetic values.  The C entry points are called on prebuilt pointer tables, so a timed window holds the launches of
one call and nothing else.

HIP events after a warm-up, REPS repeats, median / min / max.  Every timed window is preceded by a device-side fill that keeps
the stream busy while the host enqueues: the events then bracket back-to-back kernels, not the host.

  adamw_step            mc_adamw_step                                      28 B per element (30 B with a bf16 image)
  adamw_step_ema        mc_adamw_step_ema: the shadow in the same pass     +8 B
  adamw_then_ema        mc_adamw_step, then mc_ema_update                  +12 B (the parameter is read a second time)
  ema_update            mc_ema_update alone                                12 B

Each of them without bf16 images and with an image for every parameter of two or more dimensions (what the forward keeps).
GB/s figures are the algorithmic bytes above over the median time.  Prints one JSON line.

    python scripts/ema_bench.py [--reps 10] [--encoder tf_efficientnet_b5_ns-detect]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mammo_clip_amd import lib as L, ops  # noqa: E402
from mammo_clip_amd.breastclip.model import build_model  # noqa: E402


def parameter_shapes(encoder):
    cfg = {"name": "clip_custom", "temperature": 0.07,
           "image_encoder": {"source": "cnn", "name": encoder, "pretrained": True, "model_type": "cnn"},
           "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                            "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
           "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
    loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
    model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996))
    return [tuple(p.shape) for p in model.parameters()]


def event_us(fn, reps, lead, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(4):
            lead.fill_(0.0)                    # ~3 ms of device work for the host to enqueue behind
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return us


def stats(us, nbytes):
    med = statistics.median(us)
    return {"median_us": round(med, 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "reps": len(us),
            "gbps": round(nbytes / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--encoder", default="tf_efficientnet_b5_ns-detect")
    args = ap.parse_args()
    dev = torch.device("cuda")
    L.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = parameter_shapes(args.encoder)

    def rand(scale):
        return [torch.randn(s, device=dev, generator=gen) * scale for s in shapes]
    p, g, m, e = rand(0.02), rand(1e-3), rand(1e-4), rand(0.02)
    v = [x * x for x in rand(1e-3)]
    img = [torch.empty(x.shape, dtype=ops.BF16, device=dev) if x.dim() >= 2 else None for x in p]
    n = sum(x.numel() for x in p)
    n_img = sum(x.numel() for x in img if x is not None)
    cnt = len(p)

    def table(with_images):
        arr = (L.AdamwTensor * cnt)()
        for a, pp, gg, mm, vv, im in zip(arr, p, g, m, v, img):
            a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.numel = pp.data_ptr(), gg.data_ptr(), mm.data_ptr(), vv.data_ptr(), pp.numel()
            a.bf16_image = im.data_ptr() if with_images and im is not None else None
        return arr
    sh = (ctypes.c_void_p * cnt)(*[x.data_ptr() for x in e])
    src = (ctypes.c_void_p * cnt)(*[x.data_ptr() for x in p])
    numel = (ctypes.c_longlong * cnt)(*[x.numel() for x in p])
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    hyper = (1e-6, 0.9, 0.999, 1e-8, 1e-4, 10)                             # lr small: repeated steps leave the values in range
    decay, st = 0.9999, ops._st()
    lead = torch.empty(1 << 28, dtype=torch.float32, device=dev)           # 1 GiB

    def ema_update():
        L.call("mc_ema_update", sh, src, numel, cnt, decay, 1, count.data_ptr(), None, st)

    res = {"device": torch.cuda.get_device_name(0), "storage": L.STORAGE, "tensors": cnt, "elements": n, "image_elements": n_img}
    for tag, with_images in (("no_images", False), ("images", True)):
        arr = table(with_images)
        base = 28 * n + (2 * n_img if with_images else 0)

        def plain():
            L.call("mc_adamw_step", arr, cnt, *hyper, st)

        def fused():
            L.call("mc_adamw_step_ema", arr, sh, cnt, *hyper, decay, 1, count.data_ptr(), None, None, None, st)

        def sequence():
            plain()
            ema_update()
        r = {"adamw_step": stats(event_us(plain, args.reps, lead), base),
             "adamw_step_ema": stats(event_us(fused, args.reps, lead), base + 8 * n),
             "adamw_then_ema": stats(event_us(sequence, args.reps, lead), base + 12 * n)}
        r["fused_minus_plain_us"] = round(r["adamw_step_ema"]["median_us"] - r["adamw_step"]["median_us"], 1)
        r["sequence_minus_plain_us"] = round(r["adamw_then_ema"]["median_us"] - r["adamw_step"]["median_us"], 1)
        res[tag] = r
    res["ema_update"] = stats(event_us(ema_update, args.reps, lead), 12 * n)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
