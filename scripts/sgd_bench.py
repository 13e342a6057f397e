#!/usr/bin/env python3
"""Times the SGD pass of the optimizer step (optim_sgd.hip: mc_sgd_step) on the real parameter list of the flagship model,
EfficientNet-B5 + BioClinicalBERT (138 M fp32 parameters in ~700 tensors), with synthetic values, next to
torch.optim.SGD(foreach=True) on the same device and to mc_adamw_step.  The C entry points are called on prebuilt pointer
tables, so a timed window holds the launches of one call and nothing else; torch's window holds its ``step()``.

HIP events after a warm-up, REPS repeats, median / min / max.  Every timed window is preceded by a device-side fill that keeps
the stream busy while the host enqueues: the events then bracket back-to-back kernels, not the host.

  sgd_plain             mc_sgd_step, momentum 0                            12 B per element
  sgd_momentum          momentum 0.9 (a later step: the buffer is read)    20 B
  sgd_momentum_first    momentum 0.9, step 1 (the buffer is only written)  16 B
  sgd_nesterov_wd       + nesterov, weight decay                           20 B
  sgd_momentum_clip     + a clip coefficient                               20 B
  sgd_momentum_ema      + EMA shadows                                      28 B
  sgd_momentum_clip_ema + both                                             28 B
  torch_sgd_foreach     torch.optim.SGD(momentum 0.9, foreach=True).step() (its own passes over the same tensors)
  torch_sgd_plain       torch.optim.SGD(momentum 0, foreach=True).step()
  adamw_step            mc_adamw_step                                      28 B

The mc_* rows without 16-bit images and with an image for every parameter of two or more dimensions (+2 B each; what the
forward keeps).  GB/s figures are the algorithmic bytes above over the median time.  Prints one JSON line.

    python scripts/sgd_bench.py [--reps 10] [--encoder tf_efficientnet_b5_ns-detect]
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


def stats(us, nbytes=None):
    med = statistics.median(us)
    out = {"median_us": round(med, 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "reps": len(us)}
    if nbytes is not None:
        out["gbps"] = round(nbytes / med / 1e3, 1)
    return out


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
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    coef = torch.tensor([0.5], device=dev)
    lr, decay, st = 1e-6, 0.9999, ops._st()                               # lr small: repeated steps leave the values in range
    lead = torch.empty(1 << 28, dtype=torch.float32, device=dev)           # 1 GiB

    def sgd(arr, mu=0.9, wd=0.0, nesterov=0, step=10, clip=False, ema=False):
        def run():
            L.call("mc_sgd_step", arr, sh if ema else None, cnt, lr, mu, 0.0, wd, nesterov, 0, step, decay, 1, count.data_ptr(),
                   coef.data_ptr() if clip else None, None, None, st)
        return run

    res = {"device": torch.cuda.get_device_name(0), "storage": L.STORAGE, "tensors": cnt, "elements": n, "image_elements": n_img}
    for tag, with_images in (("no_images", False), ("images", True)):
        arr = table(with_images)
        extra = 2 * n_img if with_images else 0
        rows = {"sgd_plain": (sgd(arr, mu=0.0), 12), "sgd_momentum": (sgd(arr), 20), "sgd_momentum_first": (sgd(arr, step=1), 16),
                "sgd_nesterov_wd": (sgd(arr, wd=1e-4, nesterov=1), 20), "sgd_momentum_clip": (sgd(arr, clip=True), 20),
                "sgd_momentum_ema": (sgd(arr, ema=True), 28), "sgd_momentum_clip_ema": (sgd(arr, clip=True, ema=True), 28),
                "adamw_step": (lambda: L.call("mc_adamw_step", arr, cnt, lr, 0.9, 0.999, 1e-8, 1e-4, 10, st), 28)}
        res[tag] = {k: stats(event_us(fn, args.reps, lead), b * n + extra) for k, (fn, b) in rows.items()}
    # torch's own optimizer over the same tensors (parameters and gradients shared with the tables above)
    params = [torch.nn.Parameter(x) for x in p]
    for q, gg in zip(params, g):
        q.grad = gg
    for name, mu in (("torch_sgd_foreach", 0.9), ("torch_sgd_plain", 0.0)):
        opt = torch.optim.SGD(params, lr=lr, momentum=mu, foreach=True)
        res[name] = stats(event_us(opt.step, args.reps, lead))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
