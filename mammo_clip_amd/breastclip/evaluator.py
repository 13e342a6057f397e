"""Entry points of the reference's Evaluator [ref: evaluator.py:126-252]:
``encode_image`` / ``encode_text`` return L2-normalised projected embeddings (numpy arrays, or fp32 device tensors with
``as_tensor=True``), ``zeroshot_scores`` is the softmax over cosine similarities the zero-shot metrics are computed from
(evaluator.py:173).  ``retrieval_i2t`` / ``retrieve`` / ``zeroshot_metrics`` are the numbers a checkpoint is judged on
(eval_img_text_retrieval, eval_zeroshot): on device tensors they run the streamed similarity kernels of csrc/retrieval.hip
-- the N x M similarity matrix is never stored and nothing but the final scalars leaves the device -- on numpy arrays plain
numpy on the host.  No sklearn / scipy anywhere.

Out of scope: tokenising prompts, datasets and loaders, ``classification_score`` and the pF1 helpers
(evaluator.py:255-346), sharding one evaluation over several ranks, and any change to ``engine.validate``."""
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _tokens
from .model import build_model


class Evaluator:
    def __init__(self, model=None, ckpt_path: Optional[str] = None, tokenizer=None, device=None):
        """Either an already built model, or a reference-layout checkpoint (``{"model", "config", ...}``,
        trainer.py:215-237) whose ``config["model"]`` / ``config["loss"]`` rebuild it [ref: evaluator.py:24-27,52-58]."""
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if model is None:
            ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
            self.ckpt_config = ckpt["config"]
            model = build_model(self.ckpt_config["model"], self.ckpt_config["loss"], tokenizer)
            sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in ckpt["model"].items()}
            model.load_state_dict(sd, strict=False)                       # evaluator.py:151 uses strict=False
        self.model = model.to(self.device).eval()

    @torch.no_grad()
    def encode_image(self, image: torch.Tensor, as_tensor: bool = False):
        """``as_tensor=True``: the normalised fp32 embeddings stay on the device (input of the metric methods below)"""
        self.model.eval()
        emb = self.model.encode_image_normalized(image.to(self.device)).float()
        return emb.contiguous() if as_tensor else emb.cpu().numpy()

    @torch.no_grad()
    def encode_text(self, text_token: Dict, as_tensor: bool = False):
        if isinstance(text_token, (str, list)):
            raise TypeError("pass tokenised input ({'input_ids', 'attention_mask'}); tokenisation is the caller's")
        self.model.eval()
        m = self.model
        emb = m.encode_text(_tokens.to_device(text_token, self.device))
        emb = m.text_projection(emb) if m.projection else emb
        from .. import ops
        emb = ops.l2norm_fwd(emb.float().contiguous())[0]                     # the HIP normalise kernel, like encode_image
        return emb if as_tensor else emb.cpu().numpy()

    @staticmethod
    def zeroshot_scores(image_embeddings, text_embeddings) -> np.ndarray:
        """softmax over prompts of the cosine similarity [ref: evaluator.py:171].  numpy inputs (what encode_image /
        encode_text return, and what the reference computes on): host arithmetic like the reference; HIP tensors: the
        normalisation and the similarity matrix run on the device (l2norm + fp32 GEMM kernels of head.hip)."""
        if torch.is_tensor(image_embeddings) and image_embeddings.is_cuda:
            from .. import ops
            a, _ = ops.l2norm_fwd(image_embeddings.float().contiguous())
            b, _ = ops.l2norm_fwd(text_embeddings.float().contiguous().to(a.device))
            n, d = a.shape
            m = b.shape[0]
            st = torch.empty((n, m), dtype=torch.float32, device=a.device)
            ops.sgemm(a, d, 1, b, 1, d, st, m, n, m, d)                       # a @ b.T
            s = st.cpu().numpy()
        else:
            a = image_embeddings / np.linalg.norm(image_embeddings, axis=1, keepdims=True)
            b = text_embeddings / np.linalg.norm(text_embeddings, axis=1, keepdims=True)
            s = a @ b.T
        e = np.exp(s - s.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    # ---------------------------------------------------------------------------------------- metrics
    @staticmethod
    def merge_identical_texts(texts: Sequence[str]):
        """(first-occurrence index of every distinct report, label of every report among the distinct ones)
        [ref: evaluator.py:209-219, with a dict in place of the quadratic ``list.index``]"""
        first, seen, labels = [], {}, []
        for i, t in enumerate(texts):
            j = seen.get(t)
            if j is None:
                j = seen[t] = len(first)
                first.append(i)
            labels.append(j)
        return np.asarray(first, dtype=np.int64), np.asarray(labels, dtype=np.int64)

    @staticmethod
    def retrieval_i2t(image_embeddings, text_embeddings, texts: Sequence[str]) -> Dict:
        """Image-to-report retrieval [ref: evaluator.py:197-252]: ``{"retrieval_i2t": {"Recall@1", "Recall@5", "Recall@10",
        "Recall@15", "MeanRank"}}``.  Identical report strings are merged in first-occurrence order; the rank of an image's
        report is 1 + the number of distinct reports that are strictly more similar.  numpy arrays: L2-normalised here as the
        reference's cosine_similarity does, then fp64 numpy on the host.  Device tensors: the unit-norm fp32 embeddings
        ``encode_*(as_tensor=True)`` return, used in place (no normalised copy of a test set is made; rows that are not
        unit-norm raise ValueError): one ``mc_sim_rank``, the recalls and the mean rank reduced on the device."""
        first, labels = Evaluator.merge_identical_texts(texts)
        n = len(labels)
        if _on_device(image_embeddings):
            from .. import ops
            a, b = _dev_rows(image_embeddings), _dev_rows(text_embeddings, image_embeddings.device)
            assert a.shape[0] == n and b.shape[0] == n, "one text embedding and one report string per image"
            bad = _not_unit(a) + _not_unit(b)
            if len(first) < n:                                                 # (all reports distinct: b is used as it is)
                b = b.index_select(0, torch.as_tensor(first, device=a.device))
            rank = ops.sim_rank(a, b, torch.as_tensor(labels, dtype=torch.int32, device=a.device))
            ks = torch.tensor([1, 5, 10, 15], dtype=torch.int32, device=a.device)
            hits = (rank[None, :] <= ks[:, None]).sum(dim=1)                   # ranks are >= 1: every label is in range
            out = torch.cat([hits, rank.sum(dtype=torch.int64)[None], bad[None]]).cpu().numpy()   # six integers leave the device
            _raise_not_unit(out[5])
            hits, total = out[:4], int(out[4])
        else:
            a, b = _unit_np(image_embeddings), _unit_np(text_embeddings)[first]
            s = a @ b.T
            rank = 1 + (s > s[np.arange(n), labels][:, None]).sum(axis=1)
            hits, total = [(rank <= k).sum() for k in (1, 5, 10, 15)], int(rank.sum())
        result = {f"Recall@{k}": int(h) / n for k, h in zip((1, 5, 10, 15), hits)}
        result["MeanRank"] = total / n
        return {"retrieval_i2t": result}

    @staticmethod
    def retrieve(image_embeddings, text_embeddings, k: int):
        """``(scores [N, k], indices [N, k])``: the k most similar texts of every image, score descending then index ascending
        (1 <= k <= 32, k <= number of texts).  Device tensors (unit-norm fp32 rows, as in ``retrieval_i2t``; not checked here:
        nothing is read back) in, device tensors out (``mc_sim_topk``); numpy in, numpy out."""
        if _on_device(image_embeddings):
            from .. import ops
            return ops.sim_topk(_dev_rows(image_embeddings), _dev_rows(text_embeddings, image_embeddings.device), k)
        s = _unit_np(image_embeddings) @ _unit_np(text_embeddings).T
        if not 1 <= k <= min(32, s.shape[1]):
            raise ValueError("retrieve: 1 <= k <= min(32, number of texts)")
        idx = np.argsort(-s, axis=1, kind="stable")[:, :k]
        return np.take_along_axis(s, idx, axis=1), idx.astype(np.int32)

    @staticmethod
    def zeroshot_metrics(image_embeddings, prompt_embeddings: Dict, labels: Dict) -> Dict:
        """Zero-shot classification [ref: evaluator.py:160-190]: ``prompt_embeddings`` = ``{label_text: [M, D]}`` (the encoded
        prompts of one finding), ``labels`` = ``{"mass", "calc", "density", "cancer"}`` (whichever are present, one integer per
        image).  ``mass`` / ``suspicious_calcification`` / ``cancer`` / ``malignancy``: AUROC of the softmax's column 1
        against ``mass`` / ``calc`` / ``cancer`` / ``cancer``; ``density``: accuracy of the argmax.  Other keys are skipped, as
        the reference does.  AUROC is the Mann-Whitney form (pairs won + half the pairs tied) / (positives x negatives) of
        roc_curve + auc; with one class only it is NaN.  Device tensors (unit-norm fp32 rows, as in ``retrieval_i2t``):
        ``mc_sim_softmax`` + ``mc_auroc_counts``."""
        source = {"suspicious_calcification": "calc", "mass": "mass", "density": "density", "cancer": "cancer",
                  "malignancy": "cancer"}
        dev = _on_device(image_embeddings)
        if dev:
            from .. import ops
            a = _dev_rows(image_embeddings)
            bad = _not_unit(a)
        else:
            a = _unit_np(image_embeddings)
        results, pending = {}, []
        for label_text, prompts in prompt_embeddings.items():
            key = source.get(label_text.lower())
            if key is None:
                continue
            y = labels[key]
            if dev:
                b = _dev_rows(prompts, a.device)
                bad = bad + _not_unit(b)
                p = ops.sim_softmax(a, b)
                y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(a.device)
                if key == "density":
                    pending.append((label_text, None, (p.argmax(dim=1) == y).sum()))
                else:
                    pending.append((label_text, ops.auroc_counts(p[:, 1].contiguous(), y), None))
            else:
                s = a @ _unit_np(prompts).T
                e = np.exp(s - s.max(axis=1, keepdims=True))
                p = e / e.sum(axis=1, keepdims=True)
                y = np.asarray(y)
                if key == "density":
                    results[label_text] = float((p.argmax(axis=1) == y).sum()) / len(y)
                else:
                    pos, neg = p[y != 0, 1], np.sort(p[y == 0, 1])
                    lo, hi = np.searchsorted(neg, pos, side="left"), np.searchsorted(neg, pos, side="right")
                    results[label_text] = _auroc(int(lo.sum()), int((hi - lo).sum()), len(pos), len(neg))
        if dev:
            _raise_not_unit(int(bad))
        for label_text, counts, correct in pending:                           # one host read per finding, after all launches
            if counts is None:
                results[label_text] = int(correct) / a.shape[0]
            else:
                results[label_text] = _auroc(*[int(v) for v in counts.cpu()])
        return results


def _auroc(gt: int, eq: int, npos: int, nneg: int) -> float:
    return (gt + 0.5 * eq) / (npos * nneg) if npos and nneg else float("nan")


def _on_device(x) -> bool:
    return torch.is_tensor(x) and x.is_cuda


def _dev_rows(x, device=None):
    """fp32 contiguous [rows, D] on the device -- the tensor itself when it already is"""
    x = torch.as_tensor(x)
    return x.to(device=device if device is not None else x.device, dtype=torch.float32).contiguous()


def _not_unit(x):
    """device scalar: number of rows whose L2 norm is further than 1e-4 from 1 (fp32 normalisation leaves ~1e-7)"""
    return ((torch.linalg.vector_norm(x, dim=1) - 1.0).abs() > 1e-4).sum()


def _raise_not_unit(count):
    if int(count):
        raise ValueError(f"{int(count)} embedding rows are not L2-normalised: pass what encode_image / encode_text return "
                         "with as_tensor=True (or numpy arrays, which are normalised on the host)")


def _unit_np(x):
    x = np.asarray(x.cpu() if torch.is_tensor(x) else x, dtype=np.float64)
    return x / np.linalg.norm(x, axis=1, keepdims=True)
