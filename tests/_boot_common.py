"""Shared by tests/test_boot_metrics.py, tests/test_boot_metrics_gpu.py and tests/_boot_metrics_f16_worker.py: the naive
reference of a bootstrap replicate, the comparison of records against it, and the fixture tests/golden/boot_metrics.npz.

The reference does not know about bins: it builds a replicate's index array with the host Philox (``augment.philox4x32``,
one scalar counter at a time in ``naive_indices``), takes ``y[idx]`` and ``s[idx]``, and calls the numpy ``binary_metrics``
/ ``_host_curve`` / ``_host_auroc`` of the evaluator and the pair-by-pair ``brute_record`` of tests/_cls_common.py on the
resampled arrays.

Tolerances are those of tests/_cls_common.py: integers exact; metrics finished from integers 1e-12
relative; PR-AUC and AP, fp64 sums of at most K terms in [0, 1] in another order, 1e-10 absolute (K 2^-53 < 1e-12 here)."""
import math
import os

import numpy as np

import _cls_common as C
from mammo_clip_amd import augment
from mammo_clip_amd.breastclip import evaluator as EV

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "boot_metrics.npz")
THRESHOLD = 0.3          # not an fp32 value, as in tests/test_cls_metrics_gpu.py
STREAM = 0x626F6F74
GOLDEN_TAGS = tuple(f"{kind}{n}" for n in (131, 600) for kind in ("distinct", "ties"))
GOLDEN_REPLICATES, GOLDEN_SEED = 16, 2024
SEED = (0x1234 << 32) | 77          # both key words in use
# (N, kind, stratified) of the f16-build run: the scan's seam, ties, a degenerate kind, both draws
F16_CASES = ((4099, "ties8", False), (2049, "outside", True), (257, "one_positive", False), (65, "all_equal", True))
F16_REPLICATES = 9


def naive_indices(label, n_boot, seed, stratified):
    """int64 [n_boot, N] straight from the specification: one philox4x32 call per (replicate, counter)"""
    y = np.asarray(label) != 0
    n = len(y)
    pos, neg = np.flatnonzero(y), np.flatnonzero(~y)
    out = np.empty((n_boot, n), dtype=np.int64)
    for r in range(n_boot):
        for c in range((n + 3) // 4):
            words = augment.philox4x32(c, r, STREAM, 0x5bd1e995, seed & 0xFFFFFFFF, seed >> 32)
            for k in range(4):
                t = 4 * c + k
                if t >= n:
                    break
                u = int(words[k])
                if not stratified:
                    out[r, t] = (u * n) >> 32
                elif t < len(pos):
                    out[r, t] = pos[(u * len(pos)) >> 32]
                else:
                    out[r, t] = neg[(u * len(neg)) >> 32]
    return out


def records_as_dicts(records):
    """int64 [B, 20] (host array) -> one record dict per replicate"""
    assert records.dtype == np.int64 and records.ndim == 2 and records.shape[1] == 20
    assert not records[:, 12:16].any()                                   # NaN / label counters and the spare slots
    return [EV._record_of_raw(row) for row in records]


def check_replicate(rec, score, label, idx, threshold=THRESHOLD):
    """one replicate's record against the naive reference on the resampled arrays: every integer, the threshold, the fp64
    slots, and the metrics finished from it against the numpy ``binary_metrics`` -- degenerate replicates included"""
    s, y = score[idx], label[idx]
    want, _ = C.brute_record(s, y, threshold)
    C.check_record(rec, want, len(idx))
    s64, pos = s.astype(np.float64), y != 0
    got = EV._metrics_of_record(rec)
    ref = EV.binary_metrics(y, s64, threshold)
    C.check_metrics(got, ref)
    assert C.close(got["AUROC"], EV._host_auroc(pos, s64), rel=C.REL)
    tp, fp, thr = EV._host_curve(pos, s64)
    assert rec["k"] == len(thr) and rec["n_pos"] == int(pos.sum())
    hit = thr >= threshold
    assert (rec["tp"], rec["fp"]) == ((int(tp[hit].max()), int(fp[hit].max())) if hit.any() else (0, 0))
    return got


def same_float(a, b, abs_=0.0):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= abs_


def load_golden():
    z = np.load(GOLDEN)
    fx = {}
    for tag in GOLDEN_TAGS:
        fx[tag] = dict(label=z[tag + "/label"], score=z[tag + "/score"], idx=z[tag + "/idx"].astype(np.int64),
                       auroc=z[tag + "/auroc"], ap=z[tag + "/ap"], prauc=z[tag + "/prauc"], pf=z[tag + "/pf"],
                       stratified=bool(z[tag + "/stratified"]))
    return fx


def delong_se(y, s):
    """DeLong's standard error of the AUROC in fp64: placement values V10 (per positive) and V01 (per negative)"""
    pos, neg = s[y != 0].astype(np.float64), s[y == 0].astype(np.float64)
    psi = (pos[:, None] > neg[None, :]) + 0.5 * (pos[:, None] == neg[None, :])
    v10, v01 = psi.mean(axis=1), psi.mean(axis=0)
    return math.sqrt(v10.var(ddof=1) / len(pos) + v01.var(ddof=1) / len(neg))
