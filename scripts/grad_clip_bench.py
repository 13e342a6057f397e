#!/usr/bin/env python3
"""Times the gradient-norm clip of the optimizer step (optim.hip: mc_grad_norm, mc_grads_unscale_norm_dev,
mc_adamw_step_clip) on the real parameter list of the flagship model, EfficientNet-B5 + BioClinicalBERT (138 M fp32
parameters in ~700 tensors), with synthetic gradients.

HIP events after a warm-up, REPS repeats, median / min / max.  The optimizer calls spend about as long on the host (one
pointer table over 700 tensors) as the kernels run, so every timed window is preceded by a device-side fill that keeps the
stream busy while the host enqueues: the events then bracket back-to-back kernels, not the host.

  adamw_step        AdamW.step()                                                  28 B per element
  clipped_step      ops.grad_norm_coef + AdamW.step(grad_coef=)                    32 B
  norm_pass         ops.grad_norm_coef alone (the chunk sums + the finish launch)   4 B
  ls_step           LossScaler.unscale_ + step_loss_scaled + update                36 B
  ls_clipped_step   the same with unscale_(clip=) and grad_coef=                   36 B
  unscale / unscale_norm            the two unscale entries on their own (the second ends in the finish launch), 8 B

GB/s figures are the algorithmic bytes above over the median time.  The yardstick of the norm pass is the AdamW kernel's own
rate in the same run.  Prints one JSON line.

    python scripts/grad_clip_bench.py [--reps 10] [--encoder tf_efficientnet_b5_ns-detect]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mammo_clip_amd import engine, lib as L, ops  # noqa: E402
from mammo_clip_amd.breastclip.model import build_model  # noqa: E402
from mammo_clip_amd.breastclip.optimizer import AdamW  # noqa: E402


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
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    n = sum(p.numel() for p in params)
    lead = torch.empty(1 << 28, dtype=torch.float32, device=dev)           # 1 GiB
    opt = AdamW(params, lr=1e-6, weight_decay=1e-4)
    scaler = engine.LossScaler(init_scale=1.0, dynamic=False)              # scale 1: repeated unscales leave the gradients alone
    max_norm = 1.0
    arr = ops.grad_table(params, "bench")[1]
    need = L.load().mc_grad_norm_partials(arr, len(params))
    ws = torch.zeros(need, dtype=torch.float64, device=dev)
    out2 = torch.empty(2, device=dev)
    st8 = scaler.state(dev)
    scale_flag = (st8.data_ptr(), st8.data_ptr() + 4 * scaler._FLAG)

    def clipped_step():
        opt.step(grad_coef=ops.grad_norm_coef(params, max_norm)[1:])

    def ls_step():
        scaler.unscale_(params)
        scaler.update(opt.step_loss_scaled(scaler))

    def ls_clipped_step():
        nc = scaler.unscale_(params, clip=max_norm)[1]
        scaler.update(opt.step_loss_scaled(scaler, grad_coef=nc[1:]))

    cases = [
        ("adamw_step", lambda: opt.step(), 28 * n),
        ("clipped_step", clipped_step, 32 * n),
        ("norm_pass", lambda: ops.grad_norm_coef(params, max_norm), 4 * n),
        ("ls_step", ls_step, 36 * n),
        ("ls_clipped_step", ls_clipped_step, 36 * n),
        ("unscale", lambda: L.call("mc_grads_unscale_dev", arr, len(params), *scale_flag, ops._st()), 8 * n),
        ("unscale_norm", lambda: L.call("mc_grads_unscale_norm_dev", arr, len(params), *scale_flag, ws.data_ptr(), need,
                                        max_norm, out2.data_ptr(), ops._st()), 8 * n),
    ]
    res = {"device": torch.cuda.get_device_name(0), "storage": L.STORAGE, "tensors": len(params), "elements": n,
           "norm_partials": need, "max_norm": max_norm}
    for name, fn, nbytes in cases:
        res[name] = stats(event_us(fn, args.reps, lead), nbytes)
    nc = ops.grad_norm_coef(params, max_norm)
    res["grad_norm"], res["coef"] = round(nc[0].item(), 6), round(nc[1].item(), 6)
    res["norm_pass_share_of_adamw_rate"] = round(res["norm_pass"]["gbps"] / res["adamw_step"]["gbps"], 3)
    res["fused_minus_plain_unscale_us"] = round(res["unscale_norm"]["median_us"] - res["unscale"]["median_us"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
