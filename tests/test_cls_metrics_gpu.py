"""Binary-classification metrics on the device (csrc/retrieval.hip: mc_rank_counts, mc_cls_record, mc_cls_curve): the
reference fixture through the device paths of the evaluator, and each kernel against a numpy brute force on the same fp32
scores -- every integer with ``np.array_equal``, the fp64 sums to the bounds derived in tests/_cls_common.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _cls_common as C  # noqa: E402
from mammo_clip_amd import ops  # noqa: E402
from mammo_clip_amd.breastclip import evaluator as EV  # noqa: E402

DEV = torch.device("cuda")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def fx():
    return C.load()


# ------------------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("tag", C.BINARY_TAGS)
def test_device_binary_metrics_reproduce_the_reference(fx, tag):
    c = fx["binary"][tag]
    y, s = _dev(c["label"]), _dev(c["score"])
    C.check_metrics(EV.binary_metrics(y, s, fx["threshold"]), c["ref"])
    assert C.close(EV.auroc(y, s), c["ref"]["AUROC"], rel=C.REL)
    assert C.close(EV.pfbeta_binarized(c["label"], s), c["ref"]["pF"], rel=C.REL)          # (host labels, device scores)
    assert C.close(EV.pr_auc(y, s), c["ref"]["prauc"], abs_=C.ABS)
    for beta, want in zip(fx["betas"], c["pfbeta"]):
        assert C.close(EV.pfbeta(y, s, beta), float(want), abs_=C.ABS), (beta, want)
    area, precision, recall = EV.pr_auc(y, s, get_all=True)
    assert C.close(area, c["ref"]["prauc"], abs_=C.ABS)
    assert np.array_equal(precision, c["precision"]) and np.array_equal(recall, c["recall"])


@pytest.mark.parametrize("n", [131, 600])
def test_device_dicts_average_like_the_reference(fx, n):
    own = {tag: EV.binary_metrics(_dev(c["label"]), _dev(c["score"])) for tag, c in fx["binary"].items() if tag.endswith(str(n))}
    C.check_averages(own, fx["avg"][n], EV.classification_score)


def test_device_multiclass_reproduces_the_reference(fx):
    m = fx["mc"]
    C.check_multiclass(EV.multiclass_classification(_dev(m["preds"]), _dev(m["labels"]), m["classes"]), m["ref"])


def _zeroshot_detail(fx):
    z = fx["zs"]
    image, prompts = _dev(z["image"]), {k: _dev(v) for k, v in z["prompts"].items()}
    return EV.Evaluator.zeroshot_metrics(image, prompts, z["labels"]), \
        EV.Evaluator.zeroshot_metrics(image, prompts, z["labels"], detail=True)


def test_device_zeroshot_detail_reproduces_the_reference(fx):
    plain, got = _zeroshot_detail(fx)
    assert list(got) == list(plain)
    for k in C.ZS_BINARY:
        C.check_metrics(got[k], fx["zs"]["ref"][k])
        assert got[k]["AUROC"] == plain[k]
    assert got["density"] == plain["density"]


def test_f16_build_reproduces_the_reference(fx):
    """the kernels are fp32 in both storage builds: the fixture comparison in a fresh process under MC_STORAGE=f16"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "_cls_metrics_f16_worker.py")], cwd=ROOT, capture_output=True,
                       text=True, env=dict(os.environ, MC_STORAGE="f16"), timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("CLS-F16-WORKER ")][-1][len("CLS-F16-WORKER "):])
    for tag in C.BINARY_TAGS:
        c = fx["binary"][tag]
        C.check_metrics(got[tag]["metrics"], c["ref"])
        assert np.array_equal(np.asarray(got[tag]["precision"]), c["precision"])
        assert np.array_equal(np.asarray(got[tag]["recall"]), c["recall"])
        for have, want in zip(got[tag]["pfbeta"], c["pfbeta"]):
            assert C.close(have, float(want), abs_=C.ABS)
    for k in C.ZS_BINARY:
        C.check_metrics(got["zs"][k], fx["zs"]["ref"][k])


# ------------------------------------------------------------------------------------------------ kernels
THRESHOLD = 0.3      # not an fp32 value: the kernel compares in fp64, like `pred >= threshold` on the host


def _record(score, label, counts, threshold=THRESHOLD):
    return EV._read_record(ops.cls_record(score, label, counts, threshold))


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", C.SIZES)
def test_kernels_equal_brute_force(n, kind):
    score, label = C.kernel_case(n, kind)
    want, (tp, fp, thr) = C.brute_record(score, label, THRESHOLD)
    ds, dl = _dev(score), _dev(label)
    counts = ops.rank_counts(ds, dl)
    got_counts = counts.cpu().numpy()
    assert got_counts.dtype == np.int32 and np.array_equal(got_counts.view(np.uint32), C.brute_counts(score, label))
    got = _record(ds, dl, counts)
    C.check_record(got, want, n)
    gtp, gfp, gthr = [t.cpu().numpy() for t in ops.cls_curve(ds, counts, got["k"])]
    assert gtp.dtype == gfp.dtype == np.int32 and gthr.dtype == np.float32
    assert np.array_equal(gtp, tp) and np.array_equal(gfp, fp) and np.array_equal(gthr, thr)
    # without counts: the fields that need none are the same, the others empty
    bare = _record(ds, dl, None)
    for k in ("n_pos", "n_neg", "tp", "fp", "tn", "fn", "n_nan", "n_bad_label", "clip_pos", "clip_neg"):
        assert bare[k] == got[k], k
    assert (bare["gt"], bare["eq"], bare["k"]) == (0, 0, 0) and np.isnan(bare["prauc"]) and np.isnan(bare["ap"])


def test_records_are_bit_reproducible_also_on_another_stream():
    score, label = C.kernel_case(4099, "ties8")
    score[::3] = C.kernel_case(4099, "outside")[0][::3]                   # many distinct terms in the fp64 sums, and ties
    ds, dl = _dev(score), _dev(label)

    def run():
        counts = ops.rank_counts(ds, dl)
        return counts, ops.cls_record(ds, dl, counts, THRESHOLD), ops.cls_curve(ds, counts, len(np.unique(score)))

    c0, r0, v0 = run()
    c1, r1, v1 = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c2, r2, v2 = run()
    side.synchronize()
    for c, r, v in ((c1, r1, v1), (c2, r2, v2)):
        assert torch.equal(c, c0) and torch.equal(r, r0) and all(torch.equal(a, b) for a, b in zip(v, v0))
    assert r0.dtype == torch.int64 and r0.shape == (20,) and int(r0[14]) == 0 and int(r0[15]) == 0


def test_binary_metrics_reads_back_one_record_only():
    """the device path allocates the [N, 5] counts, the record and its workspace, and brings 160 bytes to the host"""
    score, label = C.kernel_case(4099, "distinct")
    ds, dl = _dev(score), _dev(label)
    EV.binary_metrics(dl, ds)                                            # library loaded, kernels resident
    copies = []
    real = torch.Tensor.cpu

    def spy(t, *a, **k):
        copies.append(t.numel() * t.element_size())
        return real(t, *a, **k)

    torch.Tensor.cpu = spy
    try:
        got = EV.binary_metrics(dl, ds)
    finally:
        torch.Tensor.cpu = real
    assert copies == [160], copies
    C.check_metrics(got, EV.binary_metrics(label, score.astype(np.float64)))


# ------------------------------------------------------------------------------------------------ errors
def test_nan_scores_and_bad_labels_raise():
    score, label = C.kernel_case(257, "distinct")
    bad_score = score.copy()
    bad_score[[0, 256]] = np.nan
    for fn in (EV.auroc, EV.pfbeta_binarized, EV.pr_auc, EV.binary_metrics, lambda g, p: EV.pfbeta(g, p, 1),
               lambda g, p: EV.pr_auc(g, p, get_all=True)):
        with pytest.raises(ValueError, match="2 scores are NaN"):
            fn(_dev(label), _dev(bad_score))
        for dtype, values in ((np.int32, [2, -1, 7]), (np.int64, [2, -1, 2 ** 32 + 1]), (np.float32, [0.5, 2.0, np.nan])):
            bad_label = label.astype(dtype)
            bad_label[[1, 64, 256]] = values
            with pytest.raises(ValueError, match="3 labels"):
                fn(_dev(bad_label), _dev(score))
        with pytest.raises(ValueError):
            fn(_dev(label[:5]), _dev(score))
    assert EV.auroc(_dev(label.astype(bool)), _dev(score)) == EV.auroc(_dev(label.astype(np.float64)), _dev(score))


def test_wrappers_check_their_arguments():
    from mammo_clip_amd.lib import MammoClipHipError
    score, label = C.kernel_case(65, "distinct")
    ds, dl = _dev(score), _dev(label)
    counts = ops.rank_counts(ds, dl)
    for call in (lambda: ops.rank_counts(ds.double(), dl), lambda: ops.rank_counts(ds, dl[:64]),
                 lambda: ops.rank_counts(torch.as_tensor(score), dl), lambda: ops.rank_counts(ds[:0], dl[:0]),
                 lambda: ops.cls_record(ds, dl, counts[:64]), lambda: ops.cls_record(ds, dl, counts.long()),
                 lambda: ops.cls_record(ds, dl, counts, float("nan")), lambda: ops.cls_curve(ds, counts, 0),
                 lambda: ops.cls_curve(ds, counts, 66), lambda: ops.cls_curve(ds[:64], counts, 3)):
        with pytest.raises(MammoClipHipError):
            call()
