#!/usr/bin/env python3
"""DEV-ONLY generator of tests/golden/eval_metrics.npz.  Runs in the build container only (needs the reference tree, sklearn
and scipy; see make_golden.py, whose ``import_reference()`` it uses as it is).

Drives the REFERENCE's own ``Evaluator.eval_img_text_retrieval`` and ``Evaluator.eval_zeroshot`` (breastclip/evaluator.py:
146-252) on an instance made with ``Evaluator.__new__``: ``get_embeddings`` returns synthetic arrays, a fake model's
``encode_text`` returns preset prompt embeddings, the tokenizer is a stand-in and the checkpoint a temporary ``{"model": {}}``
file.  The fixture holds data only: the inputs, the report strings and the reference's result dicts.

    python tests/golden/make_golden_eval.py

Retrieval cases (t: unit-norm report embeddings, g: unit-norm Gaussian noise, labels = arange(N) % U):
  case 1  seed 0  N = 131  U = 96  D = 512  image = unit(t[label] + 10 g)
  case 2  seed 1  N = 130  U = 97  D = 40   image = unit(t[label] +  3 g)
Zero-shot case: the images of case 1, random unit prompts (M = 2 for mass / suspicious_calcification / malignancy, M = 4 for
density), random labels, seed 4.

A tie that fp32 rounding could flip would make the reference's own answer ambiguous, so the generator asserts (in fp64, every
limit 2e-6, ~20 x the largest fp32 product error on these inputs) that no image has a competitor that close to its paired
similarity, no positive / negative pair has a score gap that small and no density row a top-2 gap that small."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

LIMIT = 2e-6
CASES = {"c1": dict(seed=0, n=131, u=96, d=512, noise=10.0), "c2": dict(seed=1, n=130, u=97, d=40, noise=3.0)}
ZS = {"mass": ("mass", 2), "suspicious_calcification": ("calc", 2), "malignancy": ("cancer", 2), "density": ("density", 4)}


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def retrieval_case(seed, n, u, d, noise):
    rng = np.random.default_rng(seed)
    t = unit(rng.standard_normal((u, d)))
    g = unit(rng.standard_normal((n, d)))
    labels = np.arange(n) % u
    img = unit(t[labels] + noise * g)
    return img.astype(np.float32), t.astype(np.float32), labels


class _Tokens:
    def __init__(self, prompts):
        self.prompts = tuple(prompts)

    def to(self, device):
        return self


class _Tokenizer:
    def __call__(self, prompts, **kw):
        return _Tokens(prompts)


class _Model:
    projection = False

    def __init__(self, table):
        self.table = table

    def load_state_dict(self, sd, strict=True):
        pass

    def eval(self):
        pass

    def encode_text(self, tokens):
        return torch.as_tensor(self.table[tokens.prompts])


class _DataModule:
    tokenizer = _Tokenizer()


def reference_evaluator(emb, prompt_table):
    breastclip = make_golden.import_reference()
    from breastclip.evaluator import Evaluator
    ev = Evaluator.__new__(Evaluator)
    ev.device = torch.device("cpu")
    ev.datamodule = _DataModule()
    ev.model = _Model(prompt_table)
    ev.get_embeddings = lambda checkpoint, name: emb
    return ev


def main():
    out = {}
    ckpt = os.path.join(tempfile.mkdtemp(), "ckpt.pt")
    torch.save({"model": {}}, ckpt)
    for tag, cfg in CASES.items():
        img, t, labels = retrieval_case(**cfg)
        texts = [f"report {j:03d}: finding pattern {j * 7919 % 1000}" for j in labels]
        s = unit(img.astype(np.float64)) @ unit(t.astype(np.float64)).T
        paired = s[np.arange(len(labels)), labels]
        gap = np.abs(s - paired[:, None])
        gap[np.arange(len(labels)), labels] = np.inf
        assert gap.min() >= LIMIT, (tag, gap.min())
        emb = {"image_embeddings": img, "text_embeddings": t[labels], "texts": texts}
        res = reference_evaluator(emb, {}).eval_img_text_retrieval(ckpt, "synthetic", None)["retrieval_i2t"]
        print(tag, "smallest paired-similarity margin %.3g" % gap.min(), res)
        out[tag + "/image"], out[tag + "/text_distinct"], out[tag + "/label"] = img, t, labels.astype(np.int32)
        out[tag + "/texts"] = np.asarray(texts)
        out[tag + "/result_keys"] = np.asarray(list(res.keys()))
        out[tag + "/result_values"] = np.asarray([float(v) for v in res.values()], dtype=np.float64)

    img = out["c1/image"]
    rng = np.random.default_rng(4)      # the first seed whose smallest gap clears LIMIT with some room (3.9e-6); 0-3 have a near-tie
    table, zs_prompts, emb = {}, {}, {"image_embeddings": img}
    for key, (source, m) in ZS.items():
        prompts = tuple(f"{key} prompt {j}" for j in range(m))
        zs_prompts[key] = prompts
        table[prompts] = unit(rng.standard_normal((m, img.shape[1]))).astype(np.float32)
        emb[source] = list(rng.integers(0, m, size=img.shape[0]))
        out[f"zs/prompt/{key}"], out[f"zs/label/{source}"] = table[prompts], np.asarray(emb[source], dtype=np.int32)
        s = unit(img.astype(np.float64)) @ unit(table[prompts].astype(np.float64)).T
        p = np.exp(s) / np.exp(s).sum(axis=1, keepdims=True)
        y = np.asarray(emb[source])
        if key == "density":
            top = np.sort(p, axis=1)
            assert (top[:, -1] - top[:, -2]).min() >= LIMIT, key
        else:
            assert np.abs(p[y == 1, 1][:, None] - p[y == 0, 1][None, :]).min() >= LIMIT, key
    res = reference_evaluator(emb, table).eval_zeroshot(ckpt, "synthetic", zs_prompts, None)
    print("zeroshot", res)
    out["zs/result_keys"] = np.asarray(list(res.keys()))
    out["zs/result_values"] = np.asarray([float(v) for v in res.values()], dtype=np.float64)
    path = os.path.join(HERE, "eval_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
