"""Bootstrap records on the device (csrc/retrieval.hip: mc_boot_records) against the host path of the same specification
(breastclip/evaluator.py, itself checked against the naive reference in tests/test_boot_metrics.py): every integer slot with
``torch.equal``, PR-AUC and AP to 1e-10, the clip sums to the two paths' summation error; chunking, reproducibility, the
public functions, the argument checks and the f16 storage build.

Sizes sit around the wave (64), the workgroup of the counts sweep (256), its partner tile (2048), and the scan's 1024-bin
step, which 2049 and 4099 cross twice and four times.  A replicate is addressed by its number, so the records of B replicates
are the first B rows of a longer run: B = 1, 5 and 64 are checked against the rows of the B = 65 run that the host path
answers."""
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
import _boot_common as B  # noqa: E402
import _cls_common as C  # noqa: E402
from mammo_clip_amd import lib as L, ops  # noqa: E402
from mammo_clip_amd.breastclip import evaluator as EV  # noqa: E402

DEV = torch.device("cuda")
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2049, 4099]
REPLICATES = [1, 5, 64, 65]
SEED = B.SEED


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def check_against_host(got, score, label, n_boot, threshold, seed, stratified):
    """device records (int64 [B, 20] tensor) against the host path: integers equal, fp64 slots to their bounds"""
    n = len(score)
    want = EV._host_boot_records(label != 0, score.astype(np.float64), n_boot, threshold, seed, stratified)
    assert got.dtype == torch.int64 and got.shape == (n_boot, 20)
    assert torch.equal(got[:, :16].cpu(), torch.as_tensor(want[:, :16])), np.argwhere(got[:, :16].cpu().numpy() != want[:, :16])[:5]
    gf, wf = got[:, 16:].cpu().numpy().view(np.float64), want[:, 16:].view(np.float64)
    assert np.array_equal(np.isnan(gf), np.isnan(wf))
    assert (np.nan_to_num(np.abs(gf[:, :2] - wf[:, :2])) <= C.ABS).all(), np.nanmax(np.abs(gf[:, :2] - wf[:, :2]))
    assert (np.abs(gf[:, 2:] - wf[:, 2:]) <= n * 2.0 ** -52 * np.abs(wf[:, 2:])).all()     # n 2^-53 relative on either side


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_device_records_equal_the_host_path(n, kind):
    score, label = C.kernel_case(n, kind)
    ds, dl = _dev(score), _dev(label)
    counts = ops.rank_counts(ds, dl)
    for stratified in (False, True):
        full = ops.boot_records(ds, dl, counts, REPLICATES[-1], B.THRESHOLD, SEED, stratified)
        check_against_host(full, score, label, REPLICATES[-1], B.THRESHOLD, SEED, stratified)
        for b in REPLICATES[:-1]:
            assert torch.equal(ops.boot_records(ds, dl, counts, b, B.THRESHOLD, SEED, stratified), full[:b]), (b, stratified)


@pytest.mark.parametrize("stratified", [False, True])
def test_device_records_equal_the_naive_reference(stratified):
    """the device against the reference that knows no bins, directly: every replicate of a case with ties"""
    score, label = C.kernel_case(257, "ties8")
    score[::3] = C.kernel_case(257, "outside")[0][::3]
    ds, dl = _dev(score), _dev(label)
    records = ops.boot_records(ds, dl, ops.rank_counts(ds, dl), 12, B.THRESHOLD, SEED, stratified).cpu().numpy()
    idx = EV.bootstrap_indices(label, 12, SEED, stratified)
    for rec, row in zip(B.records_as_dicts(records), idx):
        B.check_replicate(rec, score, label, row)


def test_chunks_do_not_change_the_records():
    score, label = C.kernel_case(2049, "ties8")
    score[::3] = C.kernel_case(2049, "outside")[0][::3]
    ds, dl = _dev(score), _dev(label)
    counts = ops.rank_counts(ds, dl)
    one = [ops.boot_records(ds, dl, counts, 7, B.THRESHOLD, SEED, s) for s in (False, True)]
    whole = L.load().mc_boot_ws_bytes(2049, 7)
    try:
        for chunk in (1, 2, 3):                                            # 7, 4 and 3 chunks
            ops.boot_set_chunk(chunk)
            assert L.load().mc_boot_ws_bytes(2049, 7) < whole
            for s, want in zip((False, True), one):
                assert torch.equal(ops.boot_records(ds, dl, counts, 7, B.THRESHOLD, SEED, s), want), (chunk, s)
    finally:
        ops.boot_set_chunk(0)


def test_records_are_bit_reproducible_also_on_another_stream():
    score, label = C.kernel_case(4099, "ties8")
    score[::3] = C.kernel_case(4099, "outside")[0][::3]                   # many distinct terms in the fp64 sums, and ties
    ds, dl = _dev(score), _dev(label)
    counts = ops.rank_counts(ds, dl)

    def run(seed=SEED):
        return [ops.boot_records(ds, dl, counts, 33, B.THRESHOLD, seed, s) for s in (False, True)]

    r0, r1 = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r2 = run()
    side.synchronize()
    for r in (r1, r2):
        assert all(torch.equal(a, b) for a, b in zip(r, r0))
    other = run(SEED + 1)
    assert not torch.equal(other[0], r0[0]) and not torch.equal(other[1], r0[1])
    assert not torch.equal(r0[0], r0[1])


# ------------------------------------------------------------------------------------------------ public functions
def _close_summary(got, want, compare=False):
    assert list(got) == list(want) == list(EV.BINARY_KEYS)
    for k in got:
        assert list(got[k]) == list(want[k])
        assert got[k]["n_valid"] == want[k]["n_valid"], k
        for q in ("value", "lo", "hi", "se") + (("p_le_0",) if compare else ()):
            assert B.same_float(got[k][q], want[k][q], abs_=C.ABS), (k, q, got[k][q], want[k][q])


@pytest.mark.parametrize("kind,stratified", [("ties8", False), ("outside", True), ("one_positive", False)])
def test_bootstrap_metrics_on_the_device_equal_the_numpy_path(kind, stratified):
    score, label = C.kernel_case(600, kind)
    kw = dict(n_boot=48, threshold=B.THRESHOLD, seed=SEED, stratified=stratified, alpha=0.1)
    want = EV.bootstrap_metrics(label, score.astype(np.float64), get_all=True, **kw)
    got = EV.bootstrap_metrics(_dev(label), _dev(score), get_all=True, **kw)
    _close_summary(got, want)
    for k in EV.BINARY_KEYS:
        assert np.allclose(got[k]["replicates"], want[k]["replicates"], rtol=0, atol=C.ABS, equal_nan=True)
    if kind == "one_positive":
        assert 0 < got["AUROC"]["n_valid"] < 48
    _close_summary(EV.bootstrap_metrics(label, _dev(score), **kw), EV.bootstrap_metrics(label, score.astype(np.float64), **kw))


def test_bootstrap_compare_on_the_device_equals_the_numpy_path():
    score, label = C.kernel_case(600, "distinct")
    other = (0.5 * score + 0.5 * np.random.default_rng(5).permutation(score)).astype(np.float32)
    kw = dict(n_boot=48, threshold=B.THRESHOLD, seed=SEED, alpha=0.1)
    want = EV.bootstrap_compare(label, score.astype(np.float64), other.astype(np.float64), **kw)
    got = EV.bootstrap_compare(_dev(label), _dev(score), _dev(other), **kw)
    _close_summary(got, want, compare=True)
    same = EV.bootstrap_compare(_dev(label), _dev(score), _dev(score.copy()), **kw)
    for k in EV.BINARY_KEYS:
        assert (same[k]["value"], same[k]["lo"], same[k]["hi"]) == (0.0, 0.0, 0.0)


def test_zeroshot_detail_with_intervals_and_the_default_unchanged():
    """the ``zs`` case of the fixtures (tests/_cls_common.py: the images of eval_metrics.npz, the detail prompts of
    cls_metrics.npz; no two scores closer than 2e-6, so the fp32 device softmax orders them as the fp64 host one does)"""
    z = C.load()["zs"]
    image, prompts = _dev(z["image"]), {k: _dev(v) for k, v in z["prompts"].items()}
    plain = EV.Evaluator.zeroshot_metrics(image, prompts, z["labels"], detail=True)
    for k in C.ZS_BINARY:
        C.check_metrics(plain[k], z["ref"][k])                              # exactly the seven keys, the reference's values
    got = EV.Evaluator.zeroshot_metrics(image, prompts, z["labels"], detail=True, n_boot=32, seed=SEED, alpha=0.1)
    host = EV.Evaluator.zeroshot_metrics(z["image"], z["prompts"], z["labels"], detail=True, n_boot=32, seed=SEED, alpha=0.1)
    assert list(got) == list(plain) == list(host) and got["density"] == plain["density"]
    for k in C.ZS_BINARY:
        assert list(got[k]) == C.KEYS + ["bootstrap"]
        assert {q: got[k][q] for q in C.KEYS} == plain[k]
        _close_summary(got[k]["bootstrap"], host[k]["bootstrap"])
        assert all(got[k]["bootstrap"][q]["value"] == plain[k][q] for q in C.KEYS)
    with pytest.raises(ValueError):
        EV.Evaluator.zeroshot_metrics(image, prompts, z["labels"], n_boot=8)


# ------------------------------------------------------------------------------------------------ errors
def test_argument_checks_raise_before_any_launch(monkeypatch):
    score, label = C.kernel_case(65, "distinct")
    ds, dl = _dev(score), _dev(label)
    EV.bootstrap_metrics(dl, ds, 2)
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    big = torch.zeros((1 << 24) + 1, dtype=torch.float32, device=DEV)
    for run in (lambda: EV.bootstrap_metrics(dl, ds, 0), lambda: EV.bootstrap_metrics(dl, ds, -1),
                lambda: EV.bootstrap_metrics(dl, ds, 8, alpha=0.0), lambda: EV.bootstrap_metrics(dl, ds, 8, alpha=1.0),
                lambda: EV.bootstrap_metrics(dl[:64], ds, 8), lambda: EV.bootstrap_metrics(dl[:0], ds[:0], 8),
                lambda: EV.bootstrap_metrics(big.int(), big, 8), lambda: EV.bootstrap_compare(dl, ds, ds[:64], 8),
                lambda: EV.bootstrap_compare(dl, ds, ds, 0)):
        with pytest.raises(ValueError):
            run()
    assert calls == [], calls
    monkeypatch.undo()
    counts = ops.rank_counts(ds, dl)
    for run in (lambda: ops.boot_records(ds, dl, counts, 0), lambda: ops.boot_records(ds, dl, counts, (1 << 20) + 1),
                lambda: ops.boot_records(ds, dl, counts[:64], 4), lambda: ops.boot_records(ds, dl[:64], counts, 4),
                lambda: ops.boot_records(ds.double(), dl, counts, 4), lambda: ops.boot_records(ds, dl, counts, 4, float("nan")),
                lambda: ops.boot_set_chunk(-1), lambda: ops.boot_set_stages(0)):
        with pytest.raises(L.MammoClipHipError):
            run()
    bad = score.copy()
    bad[[0, 64]] = np.nan
    with pytest.raises(ValueError, match="2 scores are NaN"):
        EV.bootstrap_metrics(dl, _dev(bad), 4)
    with pytest.raises(ValueError, match="1 labels"):
        EV.bootstrap_metrics(_dev(np.where(np.arange(65) == 7, 2, label)), ds, 4)


# ------------------------------------------------------------------------------------------------ f16 build
def test_f16_build_gives_the_same_records():
    """the kernels are fp32 in both storage builds: one run of the kernel cases in a fresh process under MC_STORAGE=f16"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "_boot_metrics_f16_worker.py")], cwd=ROOT, capture_output=True,
                       text=True, env=dict(os.environ, MC_STORAGE="f16"), timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("BOOT-F16-WORKER ")][-1][len("BOOT-F16-WORKER "):])
    assert sorted(got) == sorted(f"{n}/{kind}/{int(s)}" for n, kind, s in B.F16_CASES)
    for n, kind, stratified in B.F16_CASES:
        score, label = C.kernel_case(n, kind)
        records = torch.as_tensor(np.asarray(got[f"{n}/{kind}/{int(stratified)}"], dtype=np.int64))
        check_against_host(records, score, label, B.F16_REPLICATES, B.THRESHOLD, SEED, stratified)
