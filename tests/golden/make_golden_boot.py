#!/usr/bin/env python3
"""DEV-ONLY generator of tests/golden/boot_metrics.npz.  Runs in the build container only (needs the reference tree and
sklearn 1.7.2; see make_golden.py, whose ``import_reference()`` it uses as it is).

    python tests/golden/make_golden_boot.py

For N in {131, 600} with about 10 % positives and the score kinds ``distinct`` (N different fp32 values) and ``ties`` (the same
quantised to 8 levels): the index arrays of 16 bootstrap replicates (``evaluator.bootstrap_indices``, seed 2024; plain for
``distinct``, stratified for ``ties``) and, on every resampled pair ``(y[idx], s[idx])``, sklearn's ``roc_auc_score``,
``average_precision_score`` and ``auc(recall, precision)`` of ``precision_recall_curve``, and the reference's own
``pfbeta_binarized`` (breastclip/evaluator.py:301-309).  The fixture holds data only: labels, scores, indices and the numbers
that came back.  The test reads it, so nothing imports sklearn at test time."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402

SIZES = (131, 600)
REPLICATES, SEED = 16, 2024


def case(index, kind, n):
    rng = np.random.default_rng(300 + index)
    y = (rng.random(n) < 0.1).astype(np.int32)
    s = rng.random(n).astype(np.float32)
    if kind == "distinct":
        assert len(np.unique(s)) == n
    else:
        s = (np.floor(s * 8) / 8).astype(np.float32)
    assert 0 < y.sum() < n
    return y, s


def main():
    from mammo_clip_amd.breastclip.evaluator import bootstrap_indices
    make_golden.import_reference()
    from breastclip import evaluator as ref
    from sklearn.metrics import auc, average_precision_score, precision_recall_curve, roc_auc_score
    out, index = {}, 0
    for n in SIZES:
        for kind in ("distinct", "ties"):
            tag = f"{kind}{n}"
            y, s = case(index, kind, n)
            index += 1
            stratified = kind == "ties"
            idx = bootstrap_indices(y, REPLICATES, SEED, stratified)
            assert idx.shape == (REPLICATES, n) and idx.min() >= 0 and idx.max() < n
            rows = []
            for row in idx:
                yy, ss = y[row], s[row].astype(np.float64)
                assert 0 < yy.sum() < n                                # sklearn and the reference need both classes
                precision, recall, _ = precision_recall_curve(yy, ss)
                rows.append((roc_auc_score(yy, ss), average_precision_score(yy, ss), auc(recall, precision),
                             ref.pfbeta_binarized(yy, ss)))
            rows = np.asarray(rows, dtype=np.float64)
            out[tag + "/label"], out[tag + "/score"], out[tag + "/idx"] = y, s, idx.astype(np.int16)
            out[tag + "/stratified"] = np.bool_(stratified)
            out[tag + "/auroc"], out[tag + "/ap"], out[tag + "/prauc"], out[tag + "/pf"] = rows.T
            print(tag, "positives", int(y.sum()), "AUROC %.4f .. %.4f" % (rows[:, 0].min(), rows[:, 0].max()))
    path = os.path.join(HERE, "boot_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
