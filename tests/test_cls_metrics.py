"""Binary-classification metrics without a GPU: the numpy paths of pfbeta / pfbeta_binarized / auroc / pr_auc /
binary_metrics / classification_score / multiclass_classification and of ``zeroshot_metrics(detail=True)`` against what the
reference's own functions (and sklearn, for the keys its callers compute) returned (tests/golden/cls_metrics.npz), edge
cases against closed-form values, and the argument checks of the new C entry points."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cls_common as C  # noqa: E402
from mammo_clip_amd import lib as L  # noqa: E402
from mammo_clip_amd.breastclip import evaluator as EV  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return C.load()


# ------------------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("tag", C.BINARY_TAGS)
def test_numpy_binary_metrics_reproduce_the_reference(fx, tag):
    c = fx["binary"][tag]
    y, s = c["label"], c["score"].astype(np.float64)
    got = EV.binary_metrics(y, s, fx["threshold"])
    C.check_metrics(got, c["ref"])
    assert C.close(EV.auroc(y, s), c["ref"]["AUROC"], rel=C.REL)
    assert C.close(EV.pfbeta_binarized(y, s), c["ref"]["pF"], rel=C.REL)
    assert C.close(EV.pr_auc(y, s), c["ref"]["prauc"], abs_=C.ABS)
    for beta, want in zip(fx["betas"], c["pfbeta"]):
        assert C.close(EV.pfbeta(y, s, beta), float(want), abs_=C.ABS), (beta, want)


@pytest.mark.parametrize("tag", C.BINARY_TAGS)
def test_numpy_pr_curve_has_sklearns_layout(fx, tag):
    c = fx["binary"][tag]
    area, precision, recall = EV.pr_auc(c["label"], c["score"].astype(np.float64), get_all=True)
    k = len(np.unique(c["score"]))
    assert len(precision) == len(recall) == k + 1 and precision[-1] == 1.0 and recall[-1] == 0.0 and recall[0] == 1.0
    assert np.array_equal(precision, c["precision"]) and np.array_equal(recall, c["recall"])
    assert C.close(area, c["ref"]["prauc"], abs_=C.ABS)


def test_fixture_cases_are_what_the_issue_asks_for(fx):
    for tag, c in fx["binary"].items():
        n, k = len(c["score"]), len(np.unique(c["score"]))
        assert c["score"].dtype == np.float32 and 0.05 < c["label"].mean() < 0.15
        assert k == (8 if tag.startswith("ties") else n)
        assert (c["score"].min() < 0 and c["score"].max() > 1) == tag.startswith("clip")


@pytest.mark.parametrize("n", [131, 600])
def test_classification_score_averages_like_the_reference(fx, n):
    findings = {tag: {k: v for k, v in c["ref"].items() if k != "AP"} for tag, c in fx["binary"].items() if tag.endswith(str(n))}
    C.check_averages(findings, fx["avg"][n], EV.classification_score)
    # and on this module's own dicts ("AP" is carried along, not averaged)
    own = {tag: EV.binary_metrics(fx["binary"][tag]["label"], fx["binary"][tag]["score"]) for tag in findings}
    C.check_averages(own, fx["avg"][n], EV.classification_score)


def test_numpy_multiclass_reproduces_the_reference(fx):
    m = fx["mc"]
    C.check_multiclass(EV.multiclass_classification(m["preds"], m["labels"], m["classes"]), m["ref"])


def test_numpy_zeroshot_detail_reproduces_the_reference(fx):
    z = fx["zs"]
    plain = EV.Evaluator.zeroshot_metrics(z["image"], z["prompts"], z["labels"])
    got = EV.Evaluator.zeroshot_metrics(z["image"], z["prompts"], z["labels"], detail=True)
    assert list(got) == list(plain)
    for k in C.ZS_BINARY:
        C.check_metrics(got[k], z["ref"][k])
        assert got[k]["AUROC"] == plain[k]
    assert got["density"] == plain["density"]


# ------------------------------------------------------------------------------------------------ closed forms
def test_perfect_and_inverted_separation():
    y = np.array([0, 0, 0, 1, 1])
    s = np.array([0.1, 0.2, 0.3, 0.7, 0.9])
    m = EV.binary_metrics(y, s)
    assert all(math.isclose(m[k], 1.0, rel_tol=1e-12) for k in C.KEYS)
    m = EV.binary_metrics(1 - y, s)            # positives 0.1 0.2 0.3: best threshold 0.1 takes everything
    assert m["AUROC"] == 0.0 and math.isclose(m["pF"], 2 * 3 / (5 + 3), rel_tol=1e-12)
    assert m["F1"] == 0.0 and m["ACC_POSITIVES"] == 0.0 and m["Accuracy"] == 0.0


def test_all_scores_equal():
    """one threshold: precision P/N at recall 1, then the closing point"""
    y = np.array([1, 0, 0, 1, 0, 0, 0, 0])
    s = np.full(8, 0.25)
    m = EV.binary_metrics(y, s)
    assert m["AUROC"] == 0.5 and m["AP"] == 2 / 8 and m["prauc"] == (2 / 8 + 1) / 2
    assert math.isclose(m["pF"], 2 * 2 / (8 + 2), rel_tol=1e-12)
    assert m["ACC_POSITIVES"] == 0.0 and m["Accuracy"] == 6 / 8 and m["F1"] == 0.0
    area, p, r = EV.pr_auc(y, s, get_all=True)
    assert p.tolist() == [0.25, 1.0] and r.tolist() == [1.0, 0.0]


def test_ties_count_half_in_auroc_and_once_in_the_curve():
    y = np.array([1, 0, 1, 0])
    s = np.array([0.5, 0.5, 0.9, 0.1])
    assert EV.auroc(y, s) == (3 + 0.5) / 4
    area, p, r = EV.pr_auc(y, s, get_all=True)
    assert p.tolist() == [2 / 4, 2 / 3, 1.0, 1.0] and r.tolist() == [1.0, 1.0, 0.5, 0.0]
    assert math.isclose(area, 0.5 * (2 / 3 + 1) / 2 + 0.5 * (1 + 1) / 2, rel_tol=1e-15)
    assert math.isclose(EV.pfbeta_binarized(y, s), 2 * 2 / (2 + 1 + 2), rel_tol=1e-12)     # threshold 0.5: tp 2, fp 1


def test_single_class_inputs():
    s = np.array([0.2, 0.6, 0.4])
    m = EV.binary_metrics(np.zeros(3, dtype=int), s)
    assert all(math.isnan(m[k]) for k in ("AUROC", "pF", "prauc", "AP", "ACC_POSITIVES"))
    assert m["Accuracy"] == 2 / 3 and m["F1"] == 0.0
    assert math.isnan(EV.pfbeta(np.zeros(3, dtype=int), s, 1)) and math.isnan(EV.pfbeta_binarized(np.zeros(3, dtype=int), s))
    assert math.isnan(EV.pr_auc(np.zeros(3, dtype=int), s))
    m = EV.binary_metrics(np.ones(3, dtype=int), s)
    assert math.isnan(m["AUROC"]) and m["prauc"] == 1.0 and m["AP"] == 1.0 and m["ACC_POSITIVES"] == 1 / 3
    assert math.isclose(m["pF"], 1.0, rel_tol=1e-12)


def test_pfbeta_clips_and_returns_zero_where_the_reference_does():
    assert EV.pfbeta(np.array([1, 0]), np.array([0.5, 0.5]), 1) == 0.5
    assert EV.pfbeta(np.array([1, 0]), np.array([2.0, -1.0]), 1) == 1.0          # clipped to 1 and 0
    assert EV.pfbeta(np.array([1, 0]), np.array([-0.5, 0.0]), 1) == 0.0          # ctp + cfp == 0
    assert EV.pfbeta(np.array([1, 0]), np.array([0.0, 0.5]), 1) == 0.0           # precision 0
    # beta weighs recall: precision 0.5, recall 0.25
    got = EV.pfbeta(np.array([1, 1, 0]), np.array([0.5, 0.0, 0.5]), 2)
    assert math.isclose(got, 5 * (0.5 * 0.25) / (4 * 0.5 + 0.25), rel_tol=1e-15)


def test_threshold_counts_a_score_equal_to_it_as_positive():
    y = np.array([1, 1, 0, 0])
    s = np.array([0.3, 0.2, 0.3, 0.1], dtype=np.float32)
    m = EV.binary_metrics(y, s, threshold=float(np.float32(0.3)))
    assert m["ACC_POSITIVES"] == 0.5 and m["Accuracy"] == 0.5 and m["F1"] == 0.5
    assert EV.binary_metrics(y, s, threshold=0.31)["F1"] == 0.0


def test_bad_inputs_raise():
    y, s = np.array([1, 0, 1]), np.array([0.2, 0.5, 0.7])
    for fn in (EV.auroc, EV.pfbeta_binarized, EV.pr_auc, EV.binary_metrics, lambda g, p: EV.pfbeta(g, p, 1)):
        with pytest.raises(ValueError, match="NaN"):
            fn(y, np.array([0.2, np.nan, 0.7]))
        with pytest.raises(ValueError, match="labels"):
            fn(np.array([1, 2, 0]), s)
        with pytest.raises(ValueError, match="labels"):
            fn(np.array([1.0, 0.5, 0.0]), s)
        with pytest.raises(ValueError):
            fn(y[:2], s)
        with pytest.raises(ValueError):
            fn(y[:0], s[:0])
    assert EV.auroc(np.array([True, False, True]), s) == EV.auroc(np.array([1.0, 0.0, 1.0]), s) == 0.5


# ------------------------------------------------------------------------------------------------ C entry points
def test_new_entry_points_validate_arguments_without_gpu():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                                    # non-null, never dereferenced: the checks come first
    cap = 1 << 24
    assert lib.mc_rank_counts(None, p, p, 4, None) != 0 and b"rank_counts" in lib.mc_last_error()
    assert lib.mc_rank_counts(p, None, p, 4, None) != 0 and lib.mc_rank_counts(p, p, None, 4, None) != 0
    assert lib.mc_rank_counts(p, p, p, 0, None) != 0 and lib.mc_rank_counts(p, p, p, cap + 1, None) != 0
    assert b"2^24" in lib.mc_last_error()
    assert lib.mc_cls_record(None, p, p, 4, 0.5, p, p, None) != 0 and b"cls_record" in lib.mc_last_error()
    assert lib.mc_cls_record(p, p, p, 4, 0.5, None, p, None) != 0 and lib.mc_cls_record(p, p, p, 4, 0.5, p, None, None) != 0
    assert lib.mc_cls_record(p, p, p, 0, 0.5, p, p, None) != 0 and lib.mc_cls_record(p, p, p, cap + 1, 0.5, p, p, None) != 0
    assert lib.mc_cls_record(p, p, p, 4, math.nan, p, p, None) != 0 and b"threshold" in lib.mc_last_error()
    assert lib.mc_cls_curve(p, None, 4, 2, p, p, p, p, None) != 0 and b"cls_curve" in lib.mc_last_error()
    assert lib.mc_cls_curve(p, p, 4, 2, p, p, p, None, None) != 0
    for n, k in ((0, 1), (cap + 1, 1), (4, 0), (4, 5)):
        assert lib.mc_cls_curve(p, p, n, k, p, p, p, p, None) != 0, (n, k)
    # workspace of the record: per-workgroup partial rows, capped -- independent of N past 2^18 samples
    assert lib.mc_cls_record_ws_bytes(0) == 0 and lib.mc_cls_record_ws_bytes(cap + 1) == 0
    assert 0 < lib.mc_cls_record_ws_bytes(1) < lib.mc_cls_record_ws_bytes(1 << 18) == lib.mc_cls_record_ws_bytes(cap) <= 1 << 18
