#!/usr/bin/env python3
"""Times ``bootstrap_metrics`` of breastclip/evaluator.py (percentile intervals of one finding's metrics, DESIGN.md section
9q) at N = 50 000 scores with 2 % positives and B = 1000 replicates.

  histogram stage   mc_boot_records with only its tables + histogram kernels (the memset of every chunk included), HIP events
  record stage      mc_boot_records with only the record scan (one workgroup per replicate), HIP events
  device            the whole ``bootstrap_metrics`` call on device tensors, wall clock around a synchronise: rank counts,
                    point record, B records, B x 160 bytes read, the host finish of B records
  b_calls           what the evaluator offered before: B calls of ``binary_metrics`` on ``torch.randint``-gathered device
                    tensors (one all-pairs sweep and one 160-byte read per replicate), wall clock
  numpy             the host path of ``bootstrap_metrics`` on the same scores

Device work is timed after a warm-up; median and spread are printed.  Prints one JSON line.  No speed is gated.

    python scripts/boot_metrics_bench.py [--n 50000] [--positives 0.02] [--boot 1000] [--reps 10] [--skip-host] [--skip-calls]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eval_metrics_bench import event_ms, stats, wall_ms  # noqa: E402
from mammo_clip_amd import lib as L, ops  # noqa: E402
from mammo_clip_amd.breastclip import evaluator as EV  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--positives", type=float, default=0.02)
    ap.add_argument("--boot", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true", help="no numpy host path")
    ap.add_argument("--skip-calls", action="store_true", help="no B-calls route")
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    n, b = args.n, args.boot
    y = (torch.rand(n, device=dev, generator=gen) < args.positives).to(torch.int32)
    s = torch.sigmoid(torch.randn(n, device=dev, generator=gen) + 1.5 * y)          # positives score higher on average
    out = {"device": torch.cuda.get_device_name(0), "n": n, "positives": int(y.sum()), "n_boot": b,
           "workspace_bytes": int(L.load().mc_boot_ws_bytes(n, b))}

    counts = ops.rank_counts(s, y)
    for stratified in (False, True):
        tag = "stratified" if stratified else "plain"
        run = lambda: ops.boot_records(s, y, counts, b, 0.5, 0, stratified)  # noqa: E731
        try:
            ops.boot_set_stages(1)
            out[f"histogram_stage_{tag}"] = stats(event_ms(run, args.reps))
            ops.boot_set_stages(2)
            out[f"record_stage_{tag}"] = stats(event_ms(run, args.reps))
        finally:
            ops.boot_set_stages(3)
        out[f"boot_records_{tag}"] = stats(event_ms(run, args.reps))
    out["histogram_stage_plain"]["draws_per_s"] = round(float(n) * b / (out["histogram_stage_plain"]["median_ms"] * 1e-3), 0)
    EV.bootstrap_metrics(y, s, b)
    out["bootstrap_metrics_device"] = stats(wall_ms(lambda: EV.bootstrap_metrics(y, s, b), args.reps))
    new = EV.bootstrap_metrics(y, s, b)
    out["result"] = new

    out["b_calls_binary_metrics_device"] = out["bootstrap_metrics_numpy"] = "not measured"
    if not args.skip_calls:
        def calls():
            g = torch.Generator(device=dev).manual_seed(1)
            for _ in range(b):
                idx = torch.randint(0, n, (n,), device=dev, generator=g)
                EV.binary_metrics(y[idx], s[idx])

        calls()
        out["b_calls_binary_metrics_device"] = stats(wall_ms(calls, 3))
    if not args.skip_host:
        hy, hs = y.cpu().numpy(), s.cpu().numpy().astype("float64")
        out["bootstrap_metrics_numpy"] = stats(wall_ms(lambda: EV.bootstrap_metrics(hy, hs, b), 3))
        host = EV.bootstrap_metrics(hy, hs, b)
        out["device_differs_from_numpy_by"] = {k: max(abs(host[k][q] - new[k][q]) for q in ("lo", "hi", "se")) for k in new}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
