"""Shared by tests/test_cls_metrics.py, tests/test_cls_metrics_gpu.py and tests/_cls_metrics_f16_worker.py: the reference
fixture tests/golden/cls_metrics.npz (made by tests/golden/make_golden_cls_metrics.py), the comparison against it, and the
numpy brute force the kernels are checked against.

Tolerances (derived): every integer is exact.  AUROC, best pF1 and the threshold scores are finished on
the host from integers with the reference's formulas -- a handful of fp64 roundings: 1e-12 relative.  PR-AUC, AP and pfbeta are
fp64 sums of at most K terms in [0, 1] in another order than numpy's: at most K 2^-53 < 1e-12 here, asserted at 1e-10
absolute.  Curve precision / recall are divisions of the same exact integers on both sides: equal bit for bit."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cls_metrics.npz")
BINARY_TAGS = tuple(f"{kind}{n}" for n in (131, 600) for kind in ("distinct", "ties", "clip"))
ZS_BINARY = {"mass": "mass", "suspicious_calcification": "calc", "malignancy": "cancer"}
KEYS = ["AUROC", "pF", "prauc", "F1", "Accuracy", "ACC_POSITIVES", "AP"]
REL, ABS = 1e-12, 1e-10


def load():
    z = np.load(GOLDEN)
    ev = np.load(os.path.join(HERE, "golden", "eval_metrics.npz"))
    fx = {"threshold": float(z["threshold"]), "betas": [float(b) for b in z["betas"]], "binary": {}, "avg": {}}
    for tag in BINARY_TAGS:
        fx["binary"][tag] = dict(label=z[tag + "/label"], score=z[tag + "/score"], precision=z[tag + "/precision"],
                                 recall=z[tag + "/recall"], pfbeta=z[tag + "/pfbeta"],
                                 ref=dict(zip([str(k) for k in z[tag + "/keys"]], [float(v) for v in z[tag + "/values"]])))
    for n in (131, 600):
        fx["avg"][n] = dict(zip([str(k) for k in z[f"avg{n}/keys"]], [float(v) for v in z[f"avg{n}/values"]]))
    fx["mc"] = dict(preds=z["mc/preds"], labels=z["mc/labels"], classes=[str(c) for c in z["mc/classes"]],
                    ref=dict(zip([str(k) for k in z["mc/keys"]], [float(v) for v in z["mc/values"]])))
    keys = list(ZS_BINARY) + ["density"]
    fx["zs"] = dict(image=ev["c1/image"], prompts={k: z["zsd/prompt/" + k] for k in keys},
                    labels={s: ev["zs/label/" + s] for s in ("mass", "calc", "cancer", "density")},
                    ref={k: dict(zip([str(q) for q in z[f"zsd/{k}/keys"]], [float(v) for v in z[f"zsd/{k}/values"]]))
                         for k in ZS_BINARY})
    return fx


def close(got, want, rel=0.0, abs_=0.0):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= max(abs_, rel * abs(want))


def check_metrics(got, ref):
    """a binary_metrics dict against a dict of reference values: exactly the seven keys, in order"""
    assert list(got) == KEYS and sorted(ref) == sorted(KEYS), (list(got), list(ref))
    for k in KEYS:
        ok = close(got[k], ref[k], abs_=ABS) if k in ("prauc", "AP") else close(got[k], ref[k], rel=REL)
        assert ok, (k, got[k], ref[k])


def check_multiclass(got, ref):
    assert list(got) == list(ref)
    for k, v in ref.items():
        assert close(got[k], v, rel=REL), (k, got[k], v)


def check_averages(findings, ref, classification_score):
    """classification_score over per-finding dicts: the reference's six averaged keys, added to the dict it returns"""
    res = classification_score({k: dict(v) for k, v in findings.items()})
    assert list(res) == list(findings) + list(ref), list(res)
    for k, v in ref.items():
        assert close(float(res[k]), v, rel=REL, abs_=ABS if k == "prauc(Avg)" else 0.0), (k, res[k], v)


# ---------------------------------------------------------------------------------------------- kernel checks
# Block extents of csrc/retrieval.hip: 64-lane waves, 256 samples per workgroup, 2048 partners per tile.  One below, at and one
# above each, and a size that spans three partner tiles.
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4099]
KINDS = ["distinct", "ties8", "all_equal", "one_positive", "one_negative", "all_positive", "all_negative", "perfect",
         "inverted", "outside"]


def kernel_case(n, kind):
    """(fp32 scores, int32 labels): about 10 % positives unless the kind says otherwise"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    score = ((rng.permutation(n) + 0.5) / n).astype(np.float32)          # n distinct values in (0, 1)
    assert len(np.unique(score)) == n
    label = (rng.random(n) < 0.1).astype(np.int32)
    if kind == "ties8":
        score = (np.floor(score * 8) / 8).astype(np.float32)
    elif kind == "all_equal":
        score[:] = 0.625
    elif kind == "one_positive":
        label[:] = 0
        label[rng.integers(n)] = 1
    elif kind == "one_negative":
        label[:] = 1
        label[rng.integers(n)] = 0
    elif kind == "all_positive":
        label[:] = 1
    elif kind == "all_negative":
        label[:] = 0
    elif kind in ("perfect", "inverted"):
        order = np.argsort(score, kind="stable")
        label[:] = 0
        k = max(1, n // 10)
        label[order[-k:] if kind == "perfect" else order[:k]] = 1       # the positives hold the highest / the lowest scores
    elif kind == "outside":
        score = (score * 2 - 0.5).astype(np.float32)
    return score, label


def brute_counts(score, label):
    """[N, 5] uint32 by comparing every pair: pos_ge, neg_ge, pos_gt, neg_gt, earlier_eq"""
    pos = label != 0
    ge, gt = score[None, :] >= score[:, None], score[None, :] > score[:, None]       # [i, j]: s_j against s_i
    earlier = np.tril(ge & ~gt, -1).sum(axis=1)
    pge, pgt = ge[:, pos].sum(axis=1), gt[:, pos].sum(axis=1)
    return np.stack([pge, ge.sum(axis=1) - pge, pgt, gt.sum(axis=1) - pgt, earlier], axis=1).astype(np.uint32)


def brute_record(score, label, threshold):
    """the record's integers from definitions (not from the count columns), the curve and the fp64 values from the curve"""
    pos = label != 0
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    sp, sn = score[pos], score[~pos]
    rec = {"n_pos": n_pos, "n_neg": n_neg, "gt": int((sp[:, None] > sn[None, :]).sum()),
           "eq": int((sp[:, None] == sn[None, :]).sum())}
    best = (0, 0, -math.inf)
    for t in np.unique(sp):                                              # ascending: `>=` keeps the higher threshold on a tie
        tp, fp = int((sp >= t).sum()), int((sn >= t).sum())
        if tp * (best[0] + best[1] + n_pos) >= best[0] * (tp + fp + n_pos):           # exact integers
            best = (tp, fp, float(t))
    rec["best_tp"], rec["best_fp"], rec["best_threshold"] = best
    hit = score.astype(np.float64) >= threshold
    rec.update(tp=int((hit & pos).sum()), fp=int((hit & ~pos).sum()), tn=int((~hit & ~pos).sum()), fn=int((~hit & pos).sum()))
    thr = np.unique(score)
    rec.update(k=len(thr), n_nan=0, n_bad_label=0)
    tp = (sp[None, :] >= thr[:, None]).sum(axis=1)
    fp = (sn[None, :] >= thr[:, None]).sum(axis=1)
    curve = (tp.astype(np.int32), fp.astype(np.int32), thr)
    if n_pos:
        p = np.append(tp / (tp + fp), 1.0)
        r = np.append(tp / n_pos, 0.0)
        rec["prauc"] = -float(np.sum(np.diff(r) * (p[1:] + p[:-1]) / 2))
        rec["ap"] = -float(np.sum(np.diff(r) * p[:-1]))
    else:
        rec["prauc"] = rec["ap"] = math.nan
    c = np.clip(score.astype(np.float64), 0.0, 1.0)
    rec["clip_pos"], rec["clip_neg"] = math.fsum(c[pos]), math.fsum(c[~pos])
    return rec, curve


INT_FIELDS = ["n_pos", "n_neg", "gt", "eq", "best_tp", "best_fp", "tp", "fp", "tn", "fn", "k", "n_nan", "n_bad_label"]


def check_record(got, want, n):
    for k in INT_FIELDS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["best_threshold"] == want["best_threshold"], (got["best_threshold"], want["best_threshold"])
    for k in ("prauc", "ap"):
        assert close(got[k], want[k], abs_=ABS), (k, got[k], want[k])
    for k in ("clip_pos", "clip_neg"):                                   # n additions of fp64 terms: n 2^-53 relative
        assert abs(got[k] - want[k]) <= n * 2.0 ** -53 * want[k], (k, got[k], want[k])
