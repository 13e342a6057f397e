"""Inputs and fp64 brute-force answers of tests/test_eval_metrics_gpu.py (numpy only, computed once per session)."""
import functools

import numpy as np

LIMIT = 2e-6          # fp64 gap below which fp32 products (error ~1e-7 on unit-norm rows) may order two scores either way
RANK_SHAPES = [(131, 96, 512), (130, 97, 40), (3, 2, 512), (1, 1, 8), (70, 2500, 64), (257, 129, 513)]


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def case(n, m, d, seed=3):
    """unit-norm fp32 texts b [m, d], labels = a random choice of the m texts, images a = unit(b[label] + 3 g) (the fixture's
    recipe: the paired text is a likely but not a certain winner), and the fp64 similarities of the fp32 inputs.  Like trained
    embeddings, texts and noise live in a subspace of min(d, 16) dimensions (dense in all d coordinates): the similarities of
    one image then spread over ~0.25 instead of ~1/sqrt(d), which keeps the share of near-ties (gap < LIMIT) among the top 33
    of a row at about 1 % -- on isotropic rows it is 5 % at d = 513 and the near-tie allowances below would not mean much."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((min(d, 16), d))
    b = unit(rng.standard_normal((m, len(q))) @ q).astype(np.float32)
    label = rng.permutation(m)[:n] if n <= m else rng.integers(0, m, size=n)
    a = unit(b[label] + 3.0 * unit(rng.standard_normal((n, len(q))) @ q)).astype(np.float32)
    s = a.astype(np.float64) @ b.astype(np.float64).T
    for x in (a, b, s):
        x.setflags(write=False)
    return a, b, label.astype(np.int32), s


def rank_answer(s, label):
    """(fp64 rank, number of competitors closer than LIMIT to the paired similarity) per row"""
    n = len(label)
    paired = s[np.arange(n), label][:, None]
    close = np.abs(s - paired) < LIMIT
    close[np.arange(n), label] = False
    return 1 + (s > paired).sum(axis=1), close.sum(axis=1)


def topk_answer(s, k):
    """(fp64 top-k indices, rows whose adjacent top-(k+1) gaps are all >= LIMIT)"""
    order = np.argsort(-s, axis=1, kind="stable")[:, :min(k + 1, s.shape[1])]
    top = np.take_along_axis(s, order, axis=1)
    return order[:, :k], (-np.diff(top, axis=1) >= LIMIT).all(axis=1)
