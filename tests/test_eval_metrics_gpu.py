"""Evaluation metrics on the device (csrc/retrieval.hip): the reference fixture through Evaluator's device paths, and each
kernel against an fp64 brute force on the same fp32 inputs.  fp32 products of unit-norm rows are within ~1e-7 of fp64, so two
scores less than 2e-6 apart may legitimately come out in either order: such rows get the stated allowance, every other row
has to match exactly, and the share of rows with an allowance is capped."""
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
import _eval_cases as C  # noqa: E402
import _eval_common as E  # noqa: E402
from mammo_clip_amd import ops  # noqa: E402
from mammo_clip_amd.breastclip.evaluator import Evaluator  # noqa: E402

DEV = torch.device("cuda")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def fx():
    return E.load()


# ------------------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_device_retrieval_reproduces_the_reference(fx, tag):
    c = fx["retrieval"][tag]
    E.check_retrieval(Evaluator.retrieval_i2t(_dev(c["image"]), _dev(c["text"]), c["texts"]), c["ref"])


def test_device_zeroshot_reproduces_the_reference(fx):
    z = fx["zs"]
    got = Evaluator.zeroshot_metrics(_dev(z["image"]), {k: _dev(v) for k, v in z["prompts"].items()}, z["labels"])
    E.check_zeroshot(got, z["ref"])


def test_f16_build_reproduces_the_reference(fx):
    """the kernels are fp32 in both storage builds: same comparison in a fresh process under MC_STORAGE=f16"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "_eval_f16_worker.py")], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, MC_STORAGE="f16"), timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("EVAL-F16-WORKER ")][-1][len("EVAL-F16-WORKER "):])
    for tag in ("c1", "c2"):
        E.check_retrieval(got[tag], fx["retrieval"][tag]["ref"])
    E.check_zeroshot(got["zs"], fx["zs"]["ref"])


def test_device_path_rejects_rows_that_are_not_unit_norm(fx):
    c = fx["retrieval"]["c2"]
    with pytest.raises(ValueError):
        Evaluator.retrieval_i2t(_dev(c["image"]), _dev(2.0 * c["text"]), c["texts"])


def test_encoders_can_leave_embeddings_on_the_device():
    """as_tensor=True: the normalised fp32 device tensor, equal to what the default returns as numpy"""
    class _Model(torch.nn.Module):
        projection = False

        def encode_image_normalized(self, image):
            return ops.l2norm_fwd(image.float().reshape(image.shape[0], -1).contiguous())[0]

        def encode_text(self, tokens):
            return tokens["input_ids"].float()

    ev = Evaluator(model=_Model(), device=DEV)
    img = torch.randn(5, 3, 4, 4, generator=torch.Generator().manual_seed(0))
    tok = {"input_ids": torch.arange(1, 25).reshape(3, 8), "attention_mask": torch.ones(3, 8, dtype=torch.long)}
    for got, ref in ((ev.encode_image(img, as_tensor=True), ev.encode_image(img)),
                     (ev.encode_text(tok, as_tensor=True), ev.encode_text(tok))):
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float32 and got.is_contiguous()
        assert isinstance(ref, np.ndarray) and np.array_equal(got.cpu().numpy(), ref)
        assert np.allclose(np.linalg.norm(ref, axis=1), 1.0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ mc_sim_rank
def _check_rank(got, s, label, cap=0.02):
    want, close = C.rank_answer(s, label)
    excused = close > 0
    print(f"rank: {excused.sum()} of {len(label)} rows have a competitor within {C.LIMIT} of the paired similarity")
    assert np.array_equal(got[~excused], want[~excused]), np.flatnonzero((got != want) & ~excused)[:10]
    assert (np.abs(got - want) <= close).all()
    assert excused.mean() <= cap, excused.mean()


@pytest.mark.parametrize("shape", C.RANK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sim_rank_matches_fp64(shape):
    a, b, label, s = C.case(*shape)
    got = ops.sim_rank(_dev(a), _dev(b), _dev(label)).cpu().numpy()
    assert got.dtype == np.int32
    _check_rank(got, s, label)


def test_sim_rank_does_not_depend_on_the_split_of_m():
    a, b, label, s = C.case(70, 2500, 64)
    try:
        got = []
        for splits in (0, 1, 3, 64):
            ops.sim_set_splits(splits)
            got.append(ops.sim_rank(_dev(a), _dev(b), _dev(label)))
    finally:
        ops.sim_set_splits(0)
    assert all(torch.equal(got[0], g) for g in got[1:])


def test_sim_rank_exact_copies_of_the_paired_text_tie():
    """appending exact copies of paired texts changes no rank: a copy ties with the paired text, and ties are not counted"""
    a, b, label, s = C.case(257, 129, 513)
    b2 = np.concatenate([b, b[label[[0, 5, 77, 200, 256]]], b[label[:40]]])
    base = ops.sim_rank(_dev(a), _dev(b), _dev(label)).cpu().numpy()
    got = ops.sim_rank(_dev(a), _dev(b2), _dev(label)).cpu().numpy()
    # a copy of ANOTHER row's paired text is an ordinary competitor: it counts where the original counted
    extra = (s[:, np.concatenate([label[[0, 5, 77, 200, 256]], label[:40]])] > s[np.arange(257), label][:, None]).sum(axis=1)
    _, close = C.rank_answer(s, label)
    assert (close == 0).all()
    assert np.array_equal(got, base + extra)
    own = np.flatnonzero(extra == 0)
    assert len(own) > 0 and np.array_equal(got[own], base[own])


def test_sim_rank_out_of_range_label_gives_minus_one():
    a, b, label, s = C.case(131, 96, 512)
    bad = label.copy()
    bad[[3, 64, 130]] = [96, -1, 2 ** 30]
    got = ops.sim_rank(_dev(a), _dev(b), _dev(bad)).cpu().numpy()
    assert got[[3, 64, 130]].tolist() == [-1, -1, -1]
    keep = np.setdiff1d(np.arange(131), [3, 64, 130])
    _check_rank(got[keep], s[keep], label[keep])


# ------------------------------------------------------------------------------------------------ mc_sim_topk
@pytest.mark.parametrize("k", [1, 15, 32])
@pytest.mark.parametrize("shape", [C.RANK_SHAPES[0], C.RANK_SHAPES[4], C.RANK_SHAPES[5]], ids=lambda s: "x".join(map(str, s)))
def test_sim_topk_matches_fp64(shape, k):
    a, b, _, s = C.case(*shape)
    vals, idx = ops.sim_topk(_dev(a), _dev(b), k)
    vals, idx = vals.cpu().numpy(), idx.cpu().numpy()
    assert vals.shape == idx.shape == (shape[0], k) and idx.dtype == np.int32
    want, clear = C.topk_answer(s, k)
    print(f"topk: {(~clear).mean():.2%} of rows have a top-{k + 1} gap below {C.LIMIT}")
    assert np.array_equal(idx[clear], want[clear])
    assert (~clear).mean() <= 0.05
    assert (idx >= 0).all() and (idx < shape[1]).all() and all(len(set(r)) == k for r in idx)
    assert np.abs(vals - np.take_along_axis(s, idx.astype(np.int64), axis=1)).max() <= 1e-6
    assert (np.diff(vals, axis=1) <= 0).all()


def test_sim_topk_equal_scores_come_in_index_order_and_splits_do_not_matter():
    """every text appears three times (copies 200 and 400 rows later, i.e. in other tiles and chunks): equal scores are
    ordered by index; the result is bit-identical for every split of M and on another stream"""
    a, b, _, s = C.case(70, 200, 64, seed=5)
    b3 = np.concatenate([b, b, b])
    da, db = _dev(a), _dev(b3)
    vals, idx = ops.sim_topk(da, db, 12)
    v, i = vals.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(v[:, 0::3], v[:, 1::3]) and np.array_equal(v[:, 0::3], v[:, 2::3])
    assert np.array_equal(i[:, 1::3], i[:, 0::3] + 200) and np.array_equal(i[:, 2::3], i[:, 0::3] + 400)
    want, clear = C.topk_answer(s, 4)
    assert np.array_equal(i[clear][:, 0::3], want[clear])
    try:
        for splits in (1, 2, 5):
            ops.sim_set_splits(splits)
            v2, i2 = ops.sim_topk(da, db, 12)
            assert torch.equal(v2, vals) and torch.equal(i2, idx), splits
    finally:
        ops.sim_set_splits(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v3, i3 = ops.sim_topk(da, db, 12)
    side.synchronize()
    assert torch.equal(v3, vals) and torch.equal(i3, idx)


def test_sim_topk_rejects_a_bad_k():
    from mammo_clip_amd.lib import MammoClipHipError
    a, b, _, _ = C.case(3, 2, 512)
    for k in (0, 3, 33):
        with pytest.raises(MammoClipHipError):
            ops.sim_topk(_dev(a), _dev(b), k)


# ------------------------------------------------------------------------------------------------ mc_auroc_counts
def _auroc_brute(score, label):
    pos, neg = score[label != 0], score[label == 0]
    return [int((pos[:, None] > neg[None, :]).sum()), int((pos[:, None] == neg[None, :]).sum()), len(pos), len(neg)]


@pytest.mark.parametrize("n", [1, 2, 197, 5000])
@pytest.mark.parametrize("kind", ["random", "eight_levels", "one_class"])
def test_auroc_counts_equal_brute_force(n, kind):
    rng = np.random.default_rng(n)
    score = rng.random(n).astype(np.float32)
    label = rng.integers(0, 2, size=n).astype(np.int32)
    if kind == "eight_levels":
        score = (np.floor(score * 8) / 8).astype(np.float32)           # ties dominate
    if kind == "one_class":
        label[:] = 1
    got = ops.auroc_counts(_dev(score), _dev(label)).cpu().numpy()
    assert got.dtype == np.int64 and got.tolist() == _auroc_brute(score, label)


def test_single_class_auroc_is_nan():
    a, b, _, _ = C.case(131, 96, 512)
    got = Evaluator.zeroshot_metrics(_dev(a), {"mass": _dev(b[:2])}, {"mass": np.zeros(131, dtype=np.int64)})
    assert np.isnan(got["mass"])


# ------------------------------------------------------------------------------------------------ mc_sim_softmax
@pytest.mark.parametrize("m", [1, 2, 4, 70])
def test_sim_softmax_matches_fp64(m):
    a, b, _, s = C.case(131, 96, 512)
    p = ops.sim_softmax(_dev(a), _dev(b[:m])).cpu().numpy().astype(np.float64)
    e = np.exp(s[:, :m] - s[:, :m].max(axis=1, keepdims=True))
    assert p.shape == (131, m)
    assert np.abs(p - e / e.sum(axis=1, keepdims=True)).max() <= 1e-6
    assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ memory
def test_similarity_matrix_is_not_materialised():
    """N = M = 4096, D = 512: the N x M fp32 matrix would be 64 MB; both calls stay below 8 MB over the inputs"""
    n, d = 4096, 512
    g = torch.Generator(device=DEV).manual_seed(0)
    t = torch.nn.functional.normalize(torch.randn(n, d, device=DEV, generator=g), dim=1)
    a = torch.nn.functional.normalize(t + 0.02 * torch.randn(n, d, device=DEV, generator=g), dim=1)
    texts = [f"report {i}" for i in range(n)]
    ops.sim_rank(a[:64], t[:64], torch.arange(64, device=DEV, dtype=torch.int32))      # library loaded, kernels resident
    rises = []
    for call in (lambda: Evaluator.retrieval_i2t(a, t, texts), lambda: Evaluator.retrieve(a, t, 15)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        out = call()
        torch.cuda.synchronize()
        rises.append(torch.cuda.max_memory_allocated() - base)
        if isinstance(out, dict):
            assert out["retrieval_i2t"]["Recall@1"] == 1.0 and out["retrieval_i2t"]["MeanRank"] == 1.0
        else:
            assert torch.equal(out[1][:, 0].cpu(), torch.arange(n, dtype=torch.int32))
        del out
    print("peak rise over the inputs, bytes:", rises)
    assert rises[0] < 8 * 2 ** 20 and rises[1] < 8 * 2 ** 20, rises
