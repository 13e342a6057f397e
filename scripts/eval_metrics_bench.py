#!/usr/bin/env python3
"""Times the evaluation metrics of breastclip/evaluator.py on the device against the path a user had before them.

  retrieval   Evaluator.retrieval_i2t at N = M = 8192, D = 512 (one mc_sim_rank, five integers leave the device)
              vs ops.sgemm into an N x M buffer, .cpu(), and the reference's per-image argsort loop (evaluator.py:226-240)
  zeroshot    Evaluator.zeroshot_metrics at N = 50 000, M = 2 (mc_sim_softmax + mc_auroc_counts)
              vs the same computation on the host: scipy softmax of sklearn cosine_similarity, roc_curve + auc
              (only where sklearn is importable; otherwise reported as not measured)

Device work is timed with HIP events after a warm-up, REPS repeats, median and spread printed; host work with a wall clock
around code that ends in a synchronise.  Prints one JSON line.

    python scripts/eval_metrics_bench.py [--n 8192] [--zs-n 50000] [--reps 10] [--skip-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mammo_clip_amd import ops  # noqa: E402
from mammo_clip_amd.breastclip.evaluator import Evaluator  # noqa: E402

F32_MATRIX_PEAK = 157.3e12      # MI355X f32-input MFMA peak = the f32 vector peak, FLOP/s


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def wall_ms(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def unit_rows(n, d, gen, dev):
    return torch.nn.functional.normalize(torch.randn(n, d, device=dev, generator=gen), dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--zs-n", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true", help="device timings only")
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "n": args.n, "d": args.d, "zs_n": args.zs_n}

    # ---- retrieval
    n, d = args.n, args.d
    t = unit_rows(n, d, gen, dev)
    a = torch.nn.functional.normalize(t + 3.0 * unit_rows(n, d, gen, dev), dim=1)
    texts = [f"report {i}" for i in range(n)]
    label = torch.arange(n, device=dev, dtype=torch.int32)
    flops = 2.0 * n * n * d
    k = stats(event_ms(lambda: ops.sim_rank(a, t, label), args.reps))
    k["tflops"] = round(flops / (k["median_ms"] * 1e-3) / 1e12, 2)
    k["share_of_f32_matrix_peak"] = round(flops / (k["median_ms"] * 1e-3) / F32_MATRIX_PEAK, 3)
    out["sim_rank_kernel"] = k
    out["retrieval_i2t_device"] = stats(wall_ms(lambda: Evaluator.retrieval_i2t(a, t, texts), args.reps))
    new = Evaluator.retrieval_i2t(a, t, texts)["retrieval_i2t"]
    st = torch.empty((n, n), dtype=torch.float32, device=dev)
    g = stats(event_ms(lambda: ops.sgemm(a, d, 1, t, 1, d, st, n, n, n, d), max(3, args.reps // 3), warmup=1))
    g["tflops"] = round(flops / (g["median_ms"] * 1e-3) / 1e12, 2)
    out["stored_matrix_sgemm_kernel"] = g
    out["topk15_kernel"] = stats(event_ms(lambda: ops.sim_topk(a, t, 15), args.reps))

    def stored_path():
        ops.sgemm(a, d, 1, t, 1, d, st, n, n, n, d)
        s = st.cpu().numpy()
        recall, mean_rank = {1: 0, 5: 0, 10: 0, 15: 0}, 0
        for i in range(n):                                      # the reference's loop, one argsort per image
            rank = n - np.argwhere(s[i].argsort() == i).ravel()[0]
            mean_rank += rank
            for kk in recall:
                recall[kk] += int(rank <= kk)
        res = {f"Recall@{kk}": v / n for kk, v in recall.items()}
        res["MeanRank"] = mean_rank / n
        return res

    if not args.skip_host:
        out["retrieval_stored_matrix_host_loop"] = stats(wall_ms(stored_path, 2))
        old = stored_path()
        out["retrieval_results_differ_by"] = {kk: abs(old[kk] - new[kk]) for kk in new}
    del st

    # ---- zero-shot
    zn = args.zs_n
    za = unit_rows(zn, d, gen, dev)
    zp = unit_rows(2, d, gen, dev)
    zy = torch.randint(0, 2, (zn,), device=dev, generator=gen)
    out["zeroshot_metrics_device"] = stats(wall_ms(lambda: Evaluator.zeroshot_metrics(za, {"mass": zp}, {"mass": zy}), args.reps))
    p = ops.sim_softmax(za, zp)
    col = p[:, 1].contiguous()
    out["sim_softmax_kernel"] = stats(event_ms(lambda: ops.sim_softmax(za, zp), args.reps))
    out["auroc_counts_kernel"] = stats(event_ms(lambda: ops.auroc_counts(col, zy), args.reps))
    new = Evaluator.zeroshot_metrics(za, {"mass": zp}, {"mass": zy})["mass"]
    out["zeroshot_host_sklearn"] = "not measured"
    if not args.skip_host:
        try:
            from scipy.special import softmax
            from sklearn import metrics
        except ImportError:
            softmax = None
        if softmax is not None:
            ha, hp, hy = za.cpu().numpy(), zp.cpu().numpy(), zy.cpu().numpy()

            def host():
                sim = softmax(metrics.pairwise.cosine_similarity(ha, hp), axis=1)
                fpr, tpr, _ = metrics.roc_curve(hy, sim[:, 1])
                return metrics.auc(fpr, tpr)

            host()
            out["zeroshot_host_sklearn"] = stats(wall_ms(host, 5))
            out["zeroshot_auroc_differs_by"] = abs(float(host()) - new)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
