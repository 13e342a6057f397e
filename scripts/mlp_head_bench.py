#!/usr/bin/env python3
"""Times one projection-head call, forward + backward, for the MLP head (csrc/head.hip + mc_sgemm), the linear head (mc_sgemm)
and the same five formula lines in torch eager on the device, at m in {32, 64, 1024}, embedding_dim in {768, 2048}, n = 512,
train mode with dropout 0.1.  The numbers go into DESIGN.md section 9m; there is no pass / fail threshold.

HIP events after a warm-up, REPS repeats, median / min / max.  A head call is a dozen short launches and about as much host
time, so every timed window is preceded by a device-side fill that keeps the stream busy while the host enqueues: the events
then bracket back-to-back kernels (the time the call occupies the device), not the host.  ``host_us`` is the host's enqueue
time of the same call (a host clock around 50 calls, the device drained before and after): what a launch-bound step pays.
Prints one JSON line.

    python scripts/mlp_head_bench.py [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mammo_clip_amd import lib as L  # noqa: E402
from mammo_clip_amd.breastclip.model.modules import LinearProjectionHead, MLPProjectionHead  # noqa: E402


class EagerMLPHead(nn.Module):
    """the five formula lines in torch eager (fp32, torch's own kernels and RNG)"""

    def __init__(self, embedding_dim, n, dropout):
        super().__init__()
        self.projection, self.fc = nn.Linear(embedding_dim, n), nn.Linear(n, n)
        self.dropout, self.layer_norm = nn.Dropout(dropout), nn.LayerNorm(n)

    def forward(self, x):
        p = self.projection(x)
        return self.layer_norm(self.dropout(self.fc(nn.functional.gelu(p))) + p)


def event_us(fn, reps, lead, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            lead.fill_(0.0)                    # device work for the host to enqueue behind
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return us


def host_us(fn, calls=50):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    t1 = time.perf_counter()                   # enqueue only
    torch.cuda.synchronize()
    return 1e6 * (t1 - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlp_head_bench.py needs a HIP device")
    dev = torch.device("cuda")
    L.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    lead = torch.empty(1 << 26, dtype=torch.float32, device=dev)           # 256 MiB
    n = 512
    res = {"device": torch.cuda.get_device_name(0), "storage": L.STORAGE, "n": n, "dropout": 0.1, "reps": args.reps, "cases": []}
    for emb in (768, 2048):
        heads = {"mlp": MLPProjectionHead(emb, n, 0.1), "linear": LinearProjectionHead(emb, n), "eager": EagerMLPHead(emb, n, 0.1)}
        for h in heads.values():
            h.to(dev).train()
        for m in (32, 64, 1024):
            x = torch.randn(m, emb, device=dev, generator=gen).requires_grad_(True)
            cot = torch.randn(m, n, device=dev, generator=gen)
            row = {"m": m, "embedding_dim": emb}
            for name, head in heads.items():
                def call(head=head):
                    x.grad = None
                    for p in head.parameters():
                        p.grad = None
                    head(x).backward(cot)

                us = event_us(call, args.reps, lead)
                row[name] = {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1),
                             "max_us": round(max(us), 1), "host_us": round(host_us(call), 1)}
            res["cases"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
