"""Bootstrap confidence intervals without a GPU: the index draw against the host Philox, the host
records against the naive reference of tests/_boot_common.py on every replicate (degenerate ones included), the interval
arithmetic against numpy, the paired comparison, sklearn's numbers on stored resamples (tests/golden/boot_metrics.npz), and
the bootstrap standard error of AUROC against DeLong's."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _boot_common as B  # noqa: E402
import _cls_common as C  # noqa: E402
from mammo_clip_amd import augment  # noqa: E402
from mammo_clip_amd.breastclip import evaluator as EV  # noqa: E402

SEED = B.SEED


# ------------------------------------------------------------------------------------------------ the draw
def test_draw_known_answers():
    n, seed = 1000, SEED
    idx = EV.bootstrap_indices(np.zeros(n, dtype=np.int32), 5, seed)
    assert idx.dtype == np.int64 and idx.shape == (5, n)
    for r, t in ((0, 0), (0, 1), (0, 3), (0, 4), (3, 998), (4, 999), (2, 517)):
        u = int(augment.philox4x32(t >> 2, r, 0x626F6F74, 0x5BD1E995, seed & 0xFFFFFFFF, seed >> 32)[t & 3])
        assert idx[r, t] == (u * n) >> 32, (r, t)
    # replicates are addressed by their number: a later block of replicates equals the same rows of one call
    assert np.array_equal(EV.bootstrap_indices(np.zeros(n), 2, seed, first=3), idx[3:])
    assert not np.array_equal(EV.bootstrap_indices(np.zeros(n), 5, seed + 1), idx)
    # the resamples do not depend on the labels unless stratified
    assert np.array_equal(EV.bootstrap_indices(np.ones(n), 5, seed), idx)


@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 257])
def test_draw_equals_the_scalar_specification(n, stratified):
    label = C.kernel_case(n, "distinct")[1]
    if n >= 3:
        label[:2] = (0, 1)
    got = EV.bootstrap_indices(label, 3, SEED, stratified)
    assert np.array_equal(got, B.naive_indices(label, 3, SEED, stratified))
    assert got.min() >= 0 and got.max() < n


@pytest.mark.parametrize("n", [1, 2, 63, 600, 50000])
def test_draw_stays_in_range_and_stratified_keeps_the_class_counts(n):
    rng = np.random.default_rng(n)
    label = (rng.random(n) < 0.1).astype(np.int32)
    for strat in (False, True):
        idx = EV.bootstrap_indices(label, 7, SEED, strat)
        assert idx.min() >= 0 and idx.max() < n
    assert (label[idx].sum(axis=1) == label.sum()).all()
    for kind in ("all_positive", "all_negative", "one_positive", "one_negative"):
        label = C.kernel_case(max(n, 2) if kind.startswith("one") else n, kind)[1]
        idx = EV.bootstrap_indices(label, 7, SEED, True)
        assert idx.min() >= 0 and idx.max() < len(label) and (label[idx].sum(axis=1) == label.sum()).all()


# ------------------------------------------------------------------------------------------------ host records
@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", [1, 2, 63, 257, 600])
def test_host_records_equal_the_naive_reference(n, kind, stratified):
    score, label = C.kernel_case(n, kind)
    n_boot = 6
    records = EV._host_boot_records(label != 0, score.astype(np.float64), n_boot, B.THRESHOLD, SEED, stratified)
    idx = B.naive_indices(label, n_boot, SEED, stratified) if n <= 63 else EV.bootstrap_indices(label, n_boot, SEED, stratified)
    for rec, row in zip(B.records_as_dicts(records), idx):
        B.check_replicate(rec, score, label, row)


def test_degenerate_replicates_give_the_same_nans_and_leave_n_valid():
    """one positive among N: (1 - 1/N)^N ~ 37 % of the replicates hold none; one negative: the same for AUROC"""
    for kind, nan_keys in (("one_positive", ("AUROC", "pF", "prauc", "ACC_POSITIVES", "AP")), ("one_negative", ("AUROC",))):
        score, label = C.kernel_case(63, kind)
        n_boot = 64
        out = EV.bootstrap_metrics(label, score.astype(np.float64), n_boot, B.THRESHOLD, SEED, get_all=True)
        idx = EV.bootstrap_indices(label, n_boot, SEED)
        records = EV._host_boot_records(label != 0, score.astype(np.float64), n_boot, B.THRESHOLD, SEED, False)
        one_class = 0
        for r, (rec, row) in enumerate(zip(B.records_as_dicts(records), idx)):
            got = B.check_replicate(rec, score, label, row)                # NaN against NaN inside
            lone = label[row].sum() in (0, len(row))
            one_class += lone
            for k in EV.BINARY_KEYS:
                assert B.same_float(out[k]["replicates"][r], got[k])
                assert math.isnan(got[k]) == (lone and k in nan_keys), (kind, r, k)
            if lone and kind == "one_positive":
                assert (rec["best_tp"], rec["best_fp"], rec["best_threshold"]) == (0, 0, -math.inf)
        assert 10 <= one_class <= 40                                        # about 0.37 * 64
        for k in EV.BINARY_KEYS:
            assert out[k]["n_valid"] == n_boot - (one_class if k in nan_keys else 0)
    # stratified replicates keep the single positive: nothing is NaN
    score, label = C.kernel_case(63, "one_positive")
    out = EV.bootstrap_metrics(label, score.astype(np.float64), 16, B.THRESHOLD, SEED, stratified=True)
    assert all(v["n_valid"] == 16 for v in out.values())
    # a single class gives NaN AUROC in the point estimate and in every replicate
    score, label = C.kernel_case(63, "all_negative")
    out = EV.bootstrap_metrics(label, score.astype(np.float64), 8, B.THRESHOLD, SEED)
    assert out["AUROC"]["n_valid"] == 0 and all(math.isnan(out["AUROC"][k]) for k in ("value", "lo", "hi", "se"))
    assert out["Accuracy"]["n_valid"] == 8 and out["pF"]["n_valid"] == 0


# ------------------------------------------------------------------------------------------------ intervals
def test_intervals_equal_numpy_on_the_replicates():
    score, label = C.kernel_case(257, "ties8")
    for alpha in (0.05, 0.2):
        out = EV.bootstrap_metrics(label, score.astype(np.float64), 40, B.THRESHOLD, SEED, alpha=alpha, get_all=True)
        point = EV.binary_metrics(label, score.astype(np.float64), B.THRESHOLD)
        assert list(out) == list(EV.BINARY_KEYS)
        for k, v in out.items():
            vals = v["replicates"]
            assert vals.shape == (40,) and list(v) == ["value", "lo", "hi", "se", "n_valid", "replicates"]
            lo, hi = np.nanquantile(vals, [alpha / 2, 1 - alpha / 2])
            assert (v["lo"], v["hi"], v["se"]) == (lo, hi, np.nanstd(vals, ddof=1)) and v["n_valid"] == 40
            assert v["value"] == point[k] and v["lo"] <= v["hi"]
    plain = EV.bootstrap_metrics(label, score.astype(np.float64), 40, B.THRESHOLD, SEED, alpha=0.2)
    assert all(list(v) == ["value", "lo", "hi", "se", "n_valid"] for v in plain.values())
    assert all(plain[k][q] == out[k][q] for k in plain for q in plain[k])


def test_argument_checks_and_point_estimate_errors():
    score, label = C.kernel_case(65, "distinct")
    s64 = score.astype(np.float64)
    for kw in (dict(n_boot=0), dict(n_boot=-3), dict(n_boot=2.5), dict(alpha=0.0), dict(alpha=1.0), dict(alpha=1.5)):
        with pytest.raises(ValueError, match="bootstrap"):
            EV.bootstrap_metrics(label, s64, **{"n_boot": 4, **kw})
    with pytest.raises(ValueError):
        EV.bootstrap_metrics(label[:5], s64, 4)
    with pytest.raises(ValueError):
        EV.bootstrap_metrics(label[:0], s64[:0], 4)
    bad = s64.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="1 scores are NaN"):
        EV.bootstrap_metrics(label, bad, 4)
    with pytest.raises(ValueError, match="1 labels"):
        EV.bootstrap_metrics(np.where(np.arange(65) == 7, 2, label), s64, 4)


def test_compare_is_the_difference_of_two_runs_with_one_seed():
    score, label = C.kernel_case(257, "distinct")
    a = score.astype(np.float64)
    b = np.random.default_rng(5).permutation(a) * 0.5 + a * 0.5
    kw = dict(n_boot=50, threshold=B.THRESHOLD, seed=SEED, alpha=0.1)
    ra, rb = EV.bootstrap_metrics(label, a, get_all=True, **kw), EV.bootstrap_metrics(label, b, get_all=True, **kw)
    cmp_ = EV.bootstrap_compare(label, a, b, get_all=True, **kw)
    for k in EV.BINARY_KEYS:
        d = ra[k]["replicates"] - rb[k]["replicates"]
        lo, hi = np.nanquantile(d, [0.05, 0.95])
        v = cmp_[k]
        assert np.array_equal(v["replicates"], d, equal_nan=True)
        assert (v["value"], v["lo"], v["hi"], v["se"]) == (ra[k]["value"] - rb[k]["value"], lo, hi, np.nanstd(d, ddof=1))
        assert v["n_valid"] == 50 and v["p_le_0"] == np.count_nonzero(d <= 0) / 50
    same = EV.bootstrap_compare(label, a, a.copy(), **kw)
    for k in EV.BINARY_KEYS:
        assert (same[k]["value"], same[k]["lo"], same[k]["hi"], same[k]["se"], same[k]["p_le_0"]) == (0.0, 0.0, 0.0, 0.0, 1.0)
    # replicates where either side is undefined are left out of the comparison's n_valid
    score, label = C.kernel_case(63, "one_positive")
    lone = EV.bootstrap_compare(label, score.astype(np.float64), 1.0 - score.astype(np.float64), 64, B.THRESHOLD, SEED)
    assert 24 <= lone["AUROC"]["n_valid"] <= 54 and lone["Accuracy"]["n_valid"] == 64


# ------------------------------------------------------------------------------------------------ sklearn pin
@pytest.mark.parametrize("tag", B.GOLDEN_TAGS)
def test_replicates_reproduce_sklearn_on_the_stored_resamples(tag):
    c = B.load_golden()[tag]
    idx = EV.bootstrap_indices(c["label"], B.GOLDEN_REPLICATES, B.GOLDEN_SEED, c["stratified"])
    assert np.array_equal(idx, c["idx"])
    out = EV.bootstrap_metrics(c["label"], c["score"].astype(np.float64), B.GOLDEN_REPLICATES, 0.5, B.GOLDEN_SEED,
                               stratified=c["stratified"], get_all=True)
    for r in range(B.GOLDEN_REPLICATES):
        assert C.close(out["AUROC"]["replicates"][r], float(c["auroc"][r]), rel=C.REL), r
        assert C.close(out["pF"]["replicates"][r], float(c["pf"][r]), rel=C.REL), r
        assert C.close(out["AP"]["replicates"][r], float(c["ap"][r]), abs_=C.ABS), r
        assert C.close(out["prauc"]["replicates"][r], float(c["prauc"][r]), abs_=C.ABS), r


# ------------------------------------------------------------------------------------------------ C entry points
def test_boot_entry_points_validate_arguments_without_gpu():
    import ctypes

    from mammo_clip_amd import lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) & ~15                              # non-null, never dereferenced: the checks come first
    cap, big = 1 << 24, 1 << 40

    def call(score=p, label=p, counts=p, n=4, b=3, thr=0.5, rec=p, ws=p, nbytes=big):
        return lib.mc_boot_records(score, label, counts, n, b, thr, 7, 0, rec, ws, nbytes, None)

    for kw in (dict(score=None), dict(label=None), dict(counts=None), dict(rec=None), dict(ws=None)):
        assert call(**kw) != 0 and b"boot_records" in lib.mc_last_error(), kw
    assert call(n=0) != 0 and call(n=cap + 1) != 0 and b"2^24" in lib.mc_last_error()
    assert call(b=0) != 0 and call(b=(1 << 20) + 1) != 0 and b"2^20" in lib.mc_last_error()
    assert call(thr=math.nan) != 0 and b"threshold" in lib.mc_last_error()
    assert call(nbytes=lib.mc_boot_ws_bytes(4, 3) - 1) != 0 and b"workspace" in lib.mc_last_error()
    assert call(ws=p + 4) != 0 and b"aligned" in lib.mc_last_error()
    for n, b in ((0, 1), (cap + 1, 1), (1, 0), (1, (1 << 20) + 1)):
        assert lib.mc_boot_ws_bytes(n, b) == 0, (n, b)
    # the tables (16 N bytes) plus one chunk of histograms (8 N bytes a replicate, about 64 MiB a chunk)
    assert 16 * 50000 + 8 * 50000 * 100 <= lib.mc_boot_ws_bytes(50000, 100) < lib.mc_boot_ws_bytes(50000, 1000) \
        == lib.mc_boot_ws_bytes(50000, 100000) <= 16 * 50000 + (64 << 20) + 8192
    assert lib.mc_boot_ws_bytes(cap, 1000) <= 24 * cap + 4096               # one replicate's histogram at the largest N
    two, hundred = lib.mc_boot_ws_bytes(50000, 2), lib.mc_boot_ws_bytes(50000, 100)
    try:
        assert lib.mc_boot_set_chunk(2) == 0
        assert lib.mc_boot_ws_bytes(50000, 1000) == lib.mc_boot_ws_bytes(50000, 100) == two < hundred
        assert lib.mc_boot_set_chunk(-1) != 0 and lib.mc_boot_set_chunk(65536) != 0 and b"boot_set_chunk" in lib.mc_last_error()
    finally:
        assert lib.mc_boot_set_chunk(0) == 0
    assert lib.mc_boot_set_stages(0) != 0 and lib.mc_boot_set_stages(4) != 0 and lib.mc_boot_set_stages(3) == 0


# ------------------------------------------------------------------------------------------------ DeLong
def test_bootstrap_standard_error_of_auroc_matches_delong():
    """N = 400, about 20 % positives, scores N(0, 1) + y, B = 2000: the Monte-Carlo error of a standard error at B = 2000 is
    about 1 / sqrt(2 B) = 1.6 %, and the two estimators agree to a few percent at this N"""
    rng = np.random.default_rng(11)
    y = (rng.random(400) < 0.2).astype(np.int32)
    s = rng.standard_normal(400) + 1.0 * y
    out = EV.bootstrap_metrics(y, s, n_boot=2000, seed=20261021)
    ratio = out["AUROC"]["se"] / B.delong_se(y, s)
    print("bootstrap se", out["AUROC"]["se"], "DeLong se", B.delong_se(y, s), "ratio", ratio)
    assert 0.9 <= ratio <= 1.1
    assert out["AUROC"]["n_valid"] == 2000 and out["AUROC"]["lo"] < out["AUROC"]["value"] < out["AUROC"]["hi"]
