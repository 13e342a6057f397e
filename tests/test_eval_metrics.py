"""Evaluation metrics without a GPU: the numpy paths of Evaluator.retrieval_i2t / zeroshot_metrics against the result dicts
the reference's own eval_img_text_retrieval / eval_zeroshot produced (tests/golden/eval_metrics.npz), report merging, and the
argument checks of the new C entry points."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_common as E  # noqa: E402
from mammo_clip_amd import lib as L  # noqa: E402
from mammo_clip_amd.breastclip.evaluator import Evaluator  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return E.load()


@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_numpy_retrieval_reproduces_the_reference(fx, tag):
    c = fx["retrieval"][tag]
    E.check_retrieval(Evaluator.retrieval_i2t(c["image"], c["text"], c["texts"]), c["ref"])


def test_fixture_exercises_every_recall_bucket(fx):
    r = fx["retrieval"]["c1"]["ref"]
    assert 0 < r["Recall@1"] < r["Recall@5"] < r["Recall@10"] < r["Recall@15"] < 1 and r["MeanRank"] > 1


def test_numpy_zeroshot_reproduces_the_reference(fx):
    z = fx["zs"]
    E.check_zeroshot(Evaluator.zeroshot_metrics(z["image"], z["prompts"], z["labels"]), z["ref"])


def test_zeroshot_skips_unknown_keys_and_single_class_is_nan(fx):
    z = fx["zs"]
    prompts = {"Mass": z["prompts"]["mass"], "birads": z["prompts"]["density"]}
    got = Evaluator.zeroshot_metrics(z["image"], prompts, {"mass": np.ones(len(z["image"]), dtype=np.int32)})
    assert list(got) == ["Mass"] and math.isnan(got["Mass"])


def test_auroc_counts_ties_as_half():
    # column-1 probabilities rise with <a, p1 - p0>: images 0, 1 tie, image 2 is higher, image 3 lower
    p = np.array([[1.0, 0.0], [0.0, 1.0]])
    a = np.array([[0.6, 0.8], [0.6, 0.8], [0.0, 1.0], [1.0, 0.0]])
    got = Evaluator.zeroshot_metrics(a, {"cancer": p}, {"cancer": np.array([1, 0, 1, 0])})
    assert got["cancer"] == (3 + 0.5 * 1) / 4          # pairs won: (0,3) (2,1) (2,3); tied: (0,1)


def test_duplicate_reports_merge_in_first_occurrence_order():
    texts = ["b", "a", "b", "c", "a", "d", "d"]
    first, labels = Evaluator.merge_identical_texts(texts)
    assert first.tolist() == [0, 1, 3, 5] and labels.tolist() == [0, 1, 0, 2, 1, 3, 3]
    # the embedding of a merged report is its FIRST occurrence's: later copies with other embeddings are ignored
    rng = np.random.default_rng(0)
    t = rng.standard_normal((4, 16))
    text = t[labels].copy()
    text[[2, 4, 6]] = rng.standard_normal((3, 16))
    img = t[labels] + 0.01 * rng.standard_normal((7, 16))
    r = Evaluator.retrieval_i2t(img, text, texts)["retrieval_i2t"]
    assert r["Recall@1"] == 1.0 and r["MeanRank"] == 1.0


def test_numpy_retrieve_orders_by_score_then_index():
    b = np.eye(4)[[0, 1, 1, 2]]
    a = np.array([[0.0, 1.0, 0.0, 0.0]])
    scores, idx = Evaluator.retrieve(a, b, 3)
    assert idx.tolist() == [[1, 2, 0]] and scores.tolist() == [[1.0, 1.0, 0.0]]
    with pytest.raises(ValueError):
        Evaluator.retrieve(a, b, 5)


def test_new_entry_points_validate_arguments_without_gpu():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                                    # non-null, never dereferenced: the checks come first
    assert lib.mc_sim_rank(None, p, p, p, 4, 4, 4, None) != 0 and b"sim_rank" in lib.mc_last_error()
    assert lib.mc_sim_rank(p, p, p, None, 4, 4, 4, None) != 0
    assert lib.mc_sim_rank(p, p, p, p, 0, 4, 4, None) != 0
    assert lib.mc_sim_topk(p, p, None, p, 4, 4, 4, 1, p, None) != 0 and b"sim_topk" in lib.mc_last_error()
    assert lib.mc_sim_topk(p, p, p, p, 4, 4, 4, 1, None, None) != 0
    for k, m in ((0, 40), (33, 40), (5, 4)):
        assert lib.mc_sim_topk(p, p, p, p, 4, m, 4, k, p, None) != 0, (k, m)
        assert b"k " in lib.mc_last_error()
    assert lib.mc_sim_softmax(p, None, p, 4, 2, 4, None) != 0 and b"sim_softmax" in lib.mc_last_error()
    assert lib.mc_sim_softmax(p, p, p, 4, 0, 4, None) != 0
    assert lib.mc_auroc_counts(p, p, None, 4, None) != 0 and b"auroc_counts" in lib.mc_last_error()
    assert lib.mc_auroc_counts(p, p, p, 0, None) != 0
    assert lib.mc_sim_set_splits(-1) != 0 and lib.mc_sim_set_splits(65) != 0 and lib.mc_sim_set_splits(0) == 0
    # workspace of the top-k: O(N k splits), far from the N x M matrix
    assert 0 < lib.mc_sim_topk_ws_bytes(4096, 4096, 15) <= 4096 * 15 * 64 * 8 < 4096 * 4096 * 4
