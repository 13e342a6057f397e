#!/usr/bin/env python3
"""Times ``binary_metrics`` of breastclip/evaluator.py (pF1, PR-AUC, AP, AUROC and the threshold scores of one finding) on
the device against the host paths, at N = 50 000 scores with 2 % positives.

  kernels         mc_rank_counts, mc_cls_record (three launches) and mc_cls_curve, each by HIP events
  device          the whole ``binary_metrics`` call on device tensors, wall clock (two op calls + one 160-byte read)
  numpy           this repository's host path on the same scores (sort + searchsorted, fp64)
  sklearn         precision_recall_curve + auc + roc_auc_score on the host (only where sklearn imports; otherwise reported as
                  not measured).  The reference's pfbeta_binarized loop (positives x samples in Python) is not run at this size.

Device work is timed after a warm-up, REPS repeats, median and spread printed.  Prints one JSON line.  No speed is gated: the
feature stands on the scores staying on the device and on needing no sklearn.

    python scripts/cls_metrics_bench.py [--n 50000] [--positives 0.02] [--reps 10] [--skip-host]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eval_metrics_bench import event_ms, stats, wall_ms  # noqa: E402
from mammo_clip_amd import ops  # noqa: E402
from mammo_clip_amd.breastclip import evaluator as EV  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--positives", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true", help="device timings only")
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    n = args.n
    y = (torch.rand(n, device=dev, generator=gen) < args.positives).to(torch.int32)
    s = torch.sigmoid(torch.randn(n, device=dev, generator=gen) + 1.5 * y)          # positives score higher on average
    out = {"device": torch.cuda.get_device_name(0), "n": n, "positives": int(y.sum())}

    counts = ops.rank_counts(s, y)
    k = int(ops.cls_record(s, y, counts)[11])
    out["distinct_scores"] = k
    out["rank_counts_kernel"] = stats(event_ms(lambda: ops.rank_counts(s, y), args.reps))
    out["rank_counts_kernel"]["pair_compares_per_s"] = round(float(n) * n / (out["rank_counts_kernel"]["median_ms"] * 1e-3), 0)
    out["cls_record_kernels"] = stats(event_ms(lambda: ops.cls_record(s, y, counts), args.reps))
    out["cls_curve_kernels"] = stats(event_ms(lambda: ops.cls_curve(s, counts, k), args.reps))
    out["binary_metrics_device"] = stats(wall_ms(lambda: EV.binary_metrics(y, s), args.reps))
    new = EV.binary_metrics(y, s)
    out["result"] = new

    out["binary_metrics_numpy"] = out["host_sklearn"] = "not measured"
    if not args.skip_host:
        hy, hs = y.cpu().numpy(), s.cpu().numpy().astype("float64")
        out["binary_metrics_numpy"] = stats(wall_ms(lambda: EV.binary_metrics(hy, hs), args.reps))
        host = EV.binary_metrics(hy, hs)
        out["device_differs_from_numpy_by"] = {key: abs(host[key] - new[key]) for key in new}
        try:
            from sklearn.metrics import auc, precision_recall_curve, roc_auc_score
        except ImportError:
            auc = None
        if auc is not None:
            def sk():
                p, r, _ = precision_recall_curve(hy, hs)
                return auc(r, p), roc_auc_score(hy, hs)

            sk()
            out["host_sklearn"] = stats(wall_ms(sk, 5))
            area, roc = sk()
            out["device_differs_from_sklearn_by"] = {"prauc": abs(float(area) - new["prauc"]), "AUROC": abs(float(roc) - new["AUROC"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
