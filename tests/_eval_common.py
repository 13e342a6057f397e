"""Shared by tests/test_eval_metrics.py, tests/test_eval_metrics_gpu.py and tests/_eval_f16_worker.py: the reference fixture
tests/golden/eval_metrics.npz (made by tests/golden/make_golden_eval.py) and the comparison against its result dicts."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz")
ZS_SOURCE = {"mass": "mass", "suspicious_calcification": "calc", "malignancy": "cancer", "density": "density"}


def load():
    z = np.load(GOLDEN)
    fx = {"retrieval": {}}
    for tag in ("c1", "c2"):
        label = z[tag + "/label"]
        fx["retrieval"][tag] = dict(image=z[tag + "/image"], text=z[tag + "/text_distinct"][label], label=label,
                                    texts=[str(t) for t in z[tag + "/texts"]],
                                    ref=dict(zip([str(k) for k in z[tag + "/result_keys"]], z[tag + "/result_values"])))
    fx["zs"] = dict(image=z["c1/image"], prompts={k: z["zs/prompt/" + k] for k in ZS_SOURCE},
                    labels={s: z["zs/label/" + s] for s in set(ZS_SOURCE.values())},
                    ref=dict(zip([str(k) for k in z["zs/result_keys"]], z["zs/result_values"])))
    return fx


def check_retrieval(got, ref):
    """recalls exactly, mean rank to 1e-12"""
    got = got["retrieval_i2t"]
    assert list(got) == ["Recall@1", "Recall@5", "Recall@10", "Recall@15", "MeanRank"] == list(ref)
    for k in ("Recall@1", "Recall@5", "Recall@10", "Recall@15"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert abs(got["MeanRank"] - ref["MeanRank"]) <= 1e-12, (got["MeanRank"], ref["MeanRank"])


def check_zeroshot(got, ref):
    """AUROC and accuracy to 1e-12"""
    assert sorted(got) == sorted(ref) and len(ref) == 4
    for k, v in ref.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
