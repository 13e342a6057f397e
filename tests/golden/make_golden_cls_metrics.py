#!/usr/bin/env python3
"""DEV-ONLY generator of tests/golden/cls_metrics.npz.  Runs in the build container only (needs the reference tree and
sklearn; see make_golden.py, whose ``import_reference()`` it uses as it is).

Drives the REFERENCE's own module-level ``pfbeta``, ``pfbeta_binarized``, ``pr_auc(get_all=True)``, ``auroc``,
``multiclass_classification`` and ``classification_score`` (breastclip/evaluator.py:255-346), and sklearn's
``average_precision_score`` / ``f1_score`` / ``accuracy_score`` / ``recall_score`` for the keys the reference takes from its
callers (``AP``, and ``F1`` / ``Accuracy`` / ``ACC_POSITIVES`` at ``pred >= 0.5``).  The fixture holds data only: labels,
scores and the numbers that came back.

    python tests/golden/make_golden_cls_metrics.py

Binary cases ``<kind><N>``, N in {131, 600}, labels = (uniform < 0.1) with seed 100 + index: about 10 % positives.  Scores are
fp32 values handed to the reference as fp64, so its running sums are fp64:
  distinct  uniform [0, 1), all N values different (asserted)
  ties      the same quantised to 8 levels
  clip      uniform [-0.5, 1.5): pfbeta clips to [0, 1]
Multi-class case: N = 131, 4 classes, random fp32 scores and one-hot labels.
Zero-shot ``detail`` case: the images of eval_metrics.npz (``c1/image``) and the labels of its ``zs`` case; prompts drawn as
make_golden_eval.py draws them, with PROMPT_SEED.  The device computes the softmax in fp32, so a score pair or a score and the
0.5 threshold closer than LIMIT could legitimately come out in the other order: the generator asserts in fp64 that no two
images' scores of a binary finding, and no score and 0.5, are closer than LIMIT = 2e-6.  PROMPT_SEED is the first seed from 4
(the seed of the ``zs`` case) for which that holds; when it is 4 the prompts ARE those of the ``zs`` case (asserted)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
from make_golden_eval import ZS, unit  # noqa: E402

LIMIT = 2e-6
PROMPT_SEED = 4
SIZES = (131, 600)
KINDS = ("distinct", "ties", "clip")
THRESHOLD = 0.5
BETAS = (1.0, 2.0)


def binary_case(index, kind, n):
    rng = np.random.default_rng(100 + index)
    y = (rng.random(n) < 0.1).astype(np.int32)
    s = rng.random(n).astype(np.float32)
    if kind == "distinct":
        assert len(np.unique(s)) == n
    elif kind == "ties":
        s = (np.floor(s * 8) / 8).astype(np.float32)
    else:
        s = (s * 2 - 0.5).astype(np.float32)
    assert 0 < y.sum() < n
    return y, s


def reference_metrics(ref, y, s64):
    """one finding's dict, the reference's own functions first, sklearn for what its callers compute"""
    from sklearn.metrics import accuracy_score, average_precision_score, f1_score, recall_score
    hit = (s64 >= THRESHOLD).astype(int)
    area, precision, recall = ref.pr_auc(y, s64, get_all=True)
    m = {"AUROC": ref.auroc(y, s64), "pF": ref.pfbeta_binarized(y, s64), "prauc": area, "F1": f1_score(y, hit),
         "Accuracy": accuracy_score(y, hit), "ACC_POSITIVES": recall_score(y, hit), "AP": average_precision_score(y, s64)}
    return {k: float(v) for k, v in m.items()}, precision, recall


def zeroshot_prompts(img, seed):
    """the draw of make_golden_eval.py: per finding the prompts, then that finding's labels, from one generator"""
    rng = np.random.default_rng(seed)
    prompts = {}
    for key, (source, m) in ZS.items():
        prompts[key] = unit(rng.standard_normal((m, img.shape[1]))).astype(np.float32)
        rng.integers(0, m, size=img.shape[0])
    return prompts


def zeroshot_scores(img, prompts):
    s = unit(img.astype(np.float64)) @ unit(prompts.astype(np.float64)).T
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def clear_of_ties(p1):
    d = np.abs(p1[:, None] - p1[None, :])
    d[np.arange(len(p1)), np.arange(len(p1))] = np.inf
    return min(d.min(), np.abs(p1 - THRESHOLD).min())


def main():
    make_golden.import_reference()
    from breastclip import evaluator as ref
    out = {"threshold": np.float64(THRESHOLD), "betas": np.asarray(BETAS), "prompt_seed": np.int64(PROMPT_SEED),
           "limit": np.float64(LIMIT)}
    index = 0
    for n in SIZES:
        findings = {}
        for kind in KINDS:
            tag = f"{kind}{n}"
            y, s = binary_case(index, kind, n)
            index += 1
            s64 = s.astype(np.float64)
            m, precision, recall = reference_metrics(ref, y, s64)
            out[tag + "/label"], out[tag + "/score"] = y, s
            out[tag + "/keys"] = np.asarray(list(m))
            out[tag + "/values"] = np.asarray(list(m.values()), dtype=np.float64)
            out[tag + "/precision"], out[tag + "/recall"] = precision.astype(np.float64), recall.astype(np.float64)
            out[tag + "/pfbeta"] = np.asarray([float(ref.pfbeta(y, s64, b)) for b in BETAS], dtype=np.float64)
            findings[tag] = {k: v for k, v in m.items() if k != "AP"}
            print(tag, "positives", int(y.sum()), "distinct scores", len(precision) - 1, m)
        avg = ref.classification_score(findings)
        avg = {k: float(v) for k, v in avg.items() if k.endswith("(Avg)")}
        out[f"avg{n}/keys"], out[f"avg{n}/values"] = np.asarray(list(avg)), np.asarray(list(avg.values()), dtype=np.float64)

    rng = np.random.default_rng(200)
    preds = rng.standard_normal((131, 4)).astype(np.float32)
    labels = np.eye(4, dtype=np.int64)[rng.integers(0, 4, size=131)]
    classes = ["fatty", "scattered", "heterogeneous", "dense"]
    res = ref.multiclass_classification(preds, labels, classes)
    out["mc/preds"], out["mc/labels"], out["mc/classes"] = preds, labels, np.asarray(classes)
    out["mc/keys"], out["mc/values"] = np.asarray(list(res)), np.asarray([float(v) for v in res.values()], dtype=np.float64)
    print("multiclass", res)

    ev = np.load(os.path.join(HERE, "eval_metrics.npz"))
    img = ev["c1/image"]
    prompts = zeroshot_prompts(img, PROMPT_SEED)
    if PROMPT_SEED == 4:
        assert all(np.array_equal(prompts[k], ev["zs/prompt/" + k]) for k in ZS)
    for key, (source, m) in ZS.items():
        out["zsd/prompt/" + key] = prompts[key]
        if key == "density":
            continue
        y = ev["zs/label/" + source]
        p1 = zeroshot_scores(img, prompts[key])[:, 1]
        gap = clear_of_ties(p1)
        assert gap >= LIMIT, (key, gap)
        met, _, _ = reference_metrics(ref, y, p1)
        out[f"zsd/{key}/keys"] = np.asarray(list(met))
        out[f"zsd/{key}/values"] = np.asarray(list(met.values()), dtype=np.float64)
        print("zeroshot detail", key, "smallest gap %.3g" % gap, met)
    path = os.path.join(HERE, "cls_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
