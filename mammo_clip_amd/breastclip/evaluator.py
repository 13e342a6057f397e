"""Entry points of the reference's Evaluator [ref: evaluator.py:126-252]:
``encode_image`` / ``encode_text`` return L2-normalised projected embeddings (numpy arrays, or fp32 device tensors with
``as_tensor=True``), ``zeroshot_scores`` is the softmax over cosine similarities the zero-shot metrics are computed from
(evaluator.py:173).  ``retrieval_i2t`` / ``retrieve`` / ``zeroshot_metrics`` are the numbers a checkpoint is judged on
(eval_img_text_retrieval, eval_zeroshot): on device tensors they run the streamed similarity kernels of csrc/retrieval.hip
-- the N x M similarity matrix is never stored and nothing but the final scalars leaves the device -- on numpy arrays plain
numpy on the host.  The module-level ``pfbeta`` / ``pfbeta_binarized`` / ``auroc`` / ``pr_auc`` / ``binary_metrics`` /
``classification_score`` / ``multiclass_classification`` [ref: evaluator.py:255-346] follow the same rule: device tensors go
through the rank-count kernels of csrc/retrieval.hip and one small record is read back, numpy arrays through a sort on the
host.  No sklearn / scipy anywhere.

Bootstrap confidence intervals (``bootstrap_metrics`` / ``bootstrap_compare`` / ``zeroshot_metrics(detail=True, n_boot=B)``;
DESIGN.md section 9q).  The specification both paths follow:

* Replicate ``r`` (0 <= r < B) is N draws ``t`` (0 <= t < N).  Draw ``t`` picks sample ``idx = (u * N) >> 32`` where ``u`` is
  word ``t & 3`` of ``philox4x32(t >> 2, r, 0x626f6f74, 0x5bd1e995; key = (seed & 0xffffffff, seed >> 32))`` -- the
  function of csrc/common_hip.h and mammo_clip_amd/augment.py.  The index is a function of (seed, r, t, N) and never of the
  scores: two score vectors bootstrapped with the same seed see the same resamples (``bootstrap_compare`` rests on this).
  The multiply-high map is not exactly uniform: index probabilities differ by at most N / 2^32 relative.
* ``stratified=True``: draws ``t < n_pos`` pick ``pos[(u * n_pos) >> 32]`` from the positives in index order, the other
  ``n_neg`` draws ``neg[(u * n_neg) >> 32]`` from the negatives: every replicate keeps the class counts.
* One replicate's result is the 20-slot record of ``ops.cls_record`` on the resampled multiset: the same integer slots
  (``n_pos``, ``n_neg``, ``gt``, ``eq``, the best-pF1 ``(tp, fp, threshold bits)``, the four counts at ``threshold``, ``k`` =
  the distinct scores present; NaN and label counters 0) and the same fp64 slots (PR-AUC, AP, the two clip sums).  A score
  absent from a replicate is no threshold of it; the start point (0, 0) has precision 1; without a positive PR-AUC and AP are
  NaN and the best candidate is (0, 0, -inf).  Both paths form it from ``bin(i)`` = the number of samples with a strictly
  smaller score (tied samples share a bin, bins ascend with the score): a replicate is a histogram over (bin, class), scanned
  from the highest bin down.  The host finishes every replicate with ``_metrics_of_record``.
* Per key: ``lo, hi = np.nanquantile(values, [alpha / 2, 1 - alpha / 2])``, ``se = np.nanstd(values, ddof=1)`` and
  ``n_valid`` = the replicates where the key is not NaN.  B x 160 bytes leave the device.

Out of scope: tokenising prompts, datasets and loaders, sharding one evaluation over several ranks, and any change to
``engine.validate``."""
import logging
import warnings
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _tokens
from .model import build_model

log = logging.getLogger(__name__)


class Evaluator:
    def __init__(self, model=None, ckpt_path: Optional[str] = None, tokenizer=None, device=None, use_ema: bool = False):
        """Either an already built model, or a reference-layout checkpoint (``{"model", "config", ...}``,
        trainer.py:215-237) whose ``config["model"]`` / ``config["loss"]`` rebuild it [ref: evaluator.py:24-27,52-58].
        ``use_ema``: load the averaged weights ``"model_ema"`` of the checkpoint (``checkpoint.save_checkpoint(ema=)``) instead
        of ``"model"``; KeyError when the file has none.  (An averaged model in memory is just a model: ``model=ema.module``.)"""
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if model is None:
            ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
            if use_ema and "model_ema" not in ckpt:
                raise KeyError(f"{ckpt_path} was saved without averaged weights (no 'model_ema')")
            self.ckpt_config = ckpt["config"]
            model = build_model(self.ckpt_config["model"], self.ckpt_config["loss"], tokenizer)
            sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in ckpt["model_ema" if use_ema else "model"].items()}
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
    def zeroshot_metrics(image_embeddings, prompt_embeddings: Dict, labels: Dict, detail: bool = False, n_boot: int = 0,
                         seed: int = 0, stratified: bool = False, alpha: float = 0.05) -> Dict:
        """Zero-shot classification [ref: evaluator.py:160-190]: ``prompt_embeddings`` = ``{label_text: [M, D]}`` (the encoded
        prompts of one finding), ``labels`` = ``{"mass", "calc", "density", "cancer"}`` (whichever are present, one integer per
        image).  ``mass`` / ``suspicious_calcification`` / ``cancer`` / ``malignancy``: AUROC of the softmax's column 1
        against ``mass`` / ``calc`` / ``cancer`` / ``cancer``; ``density``: accuracy of the argmax.  Other keys are skipped, as
        the reference does.  AUROC is the Mann-Whitney form (pairs won + half the pairs tied) / (positives x negatives) of
        roc_curve + auc; with one class only it is NaN.  Device tensors (unit-norm fp32 rows, as in ``retrieval_i2t``):
        ``mc_sim_softmax`` + ``mc_auroc_counts``.  ``detail=True``: every binary finding maps to its ``binary_metrics``
        dict (threshold 0.5) instead of the bare AUROC -- on the device ``mc_rank_counts`` + ``mc_cls_record``, one record read
        per finding.  ``n_boot > 0`` (with ``detail=True``): every binary finding's dict gains ``"bootstrap"``, the
        ``bootstrap_metrics`` dict of that finding (``seed``, ``stratified``, ``alpha`` as there; on the device
        ``mc_boot_records``, n_boot more records read per finding)."""
        if n_boot:
            if not detail:
                raise ValueError("zeroshot_metrics: n_boot > 0 needs detail=True")
            _check_boot_args(n_boot, alpha)
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
                elif detail:
                    col, y = _dev_score_label(y, p[:, 1])
                    counts = ops.rank_counts(col, y)
                    boot = ops.boot_records(col, y, counts, n_boot, 0.5, seed, stratified) if n_boot else None
                    pending.append((label_text, (ops.cls_record(col, y, counts), boot), None))
                else:
                    pending.append((label_text, ops.auroc_counts(p[:, 1].contiguous(), y), None))
            else:
                s = a @ _unit_np(prompts).T
                e = np.exp(s - s.max(axis=1, keepdims=True))
                p = e / e.sum(axis=1, keepdims=True)
                y = np.asarray(y)
                if key == "density":
                    results[label_text] = float((p.argmax(axis=1) == y).sum()) / len(y)
                elif detail:
                    results[label_text] = binary_metrics(y, p[:, 1])
                    if n_boot:
                        results[label_text]["bootstrap"] = bootstrap_metrics(y, p[:, 1], n_boot, 0.5, seed, stratified, alpha)
                else:
                    pos, neg = p[y != 0, 1], np.sort(p[y == 0, 1])
                    lo, hi = np.searchsorted(neg, pos, side="left"), np.searchsorted(neg, pos, side="right")
                    results[label_text] = _auroc(int(lo.sum()), int((hi - lo).sum()), len(pos), len(neg))
        if dev:
            _raise_not_unit(int(bad))
        for label_text, counts, correct in pending:                           # one host read per finding, after all launches
            if counts is None:
                results[label_text] = int(correct) / a.shape[0]
            elif detail:
                results[label_text] = _metrics_of_record(_read_record(counts[0]))
                if n_boot:
                    value = dict(results[label_text])
                    results[label_text]["bootstrap"] = _boot_summary(value, counts[1].cpu().numpy(), alpha, False)
            else:
                results[label_text] = _auroc(*[int(v) for v in counts.cpu()])
        return results


def _auroc(gt: int, eq: int, npos: int, nneg: int) -> float:
    return (gt + 0.5 * eq) / (npos * nneg) if npos and nneg else float("nan")


# ------------------------------------------------------------------------------- binary-classification metrics of one finding
# [ref: evaluator.py:255-346].  Everything is finished from exact integers: (TP, FP) at every distinct threshold.  On device
# tensors they come from the all-pairs rank counts of csrc/retrieval.hip; on numpy arrays from a sort and
# searchsorted in fp64.  A NaN score or a label outside {0, 1} raises ValueError on both paths.
BINARY_KEYS = ("AUROC", "pF", "prauc", "F1", "Accuracy", "ACC_POSITIVES", "AP")
_NAN = float("nan")


def pfbeta(gt, pred, beta) -> float:
    """Probabilistic F-beta on scores clipped to [0, 1] [ref: evaluator.py:316-337]: ctp / cfp are the sums of the clipped
    scores over positives / negatives.  0.0 when ctp + cfp == 0 or precision or recall is 0; NaN without a positive (the
    reference divides by zero there)."""
    if _on_device(pred):
        from .. import ops
        score, label = _dev_score_label(gt, pred)
        rec = _read_record(ops.cls_record(score, label, None))
        n_pos, ctp, cfp = rec["n_pos"], rec["clip_pos"], rec["clip_neg"]
    else:
        y, s = _host_score_label(gt, pred)
        c = np.clip(s, 0.0, 1.0)
        n_pos, ctp, cfp = int(y.sum()), float(c[y].sum()), float(c[~y].sum())
    if n_pos == 0:
        return _NAN
    if ctp + cfp == 0:
        return 0.0
    b2 = beta * beta
    p, r = ctp / (ctp + cfp), ctp / n_pos
    return (1 + b2) * (p * r) / (b2 * p + r) if p > 0 and r > 0 else 0.0


def pfbeta_binarized(gt, pred) -> float:
    """The best pF1 of ``pred >= th`` over the thresholds ``th`` taken from the positives' scores [ref: evaluator.py:301-309,
    without its positives x samples loop]; NaN without a positive (the reference raises on ``max([])``)."""
    if _on_device(pred):
        from .. import ops
        score, label = _dev_score_label(gt, pred)
        rec = _read_record(ops.cls_record(score, label, ops.rank_counts(score, label)))
        return _pf1(rec["best_tp"], rec["best_fp"], rec["n_pos"])
    y, s = _host_score_label(gt, pred)
    return _host_best_pf1(y, s)


def auroc(gt, pred) -> float:
    """roc_auc_score in its Mann-Whitney form (pairs won + half the pairs tied) / (positives x negatives)
    [ref: evaluator.py:312-313]; NaN with one class only"""
    if _on_device(pred):
        from .. import ops
        score, label = _dev_score_label(gt, pred)
        rec = _read_record(ops.cls_record(score, label, ops.rank_counts(score, label)))
        return _auroc(rec["gt"], rec["eq"], rec["n_pos"], rec["n_neg"])
    y, s = _host_score_label(gt, pred)
    return _host_auroc(y, s)


def pr_auc(gt, pred, get_all=False):
    """The trapezoid under sklearn's precision_recall_curve [ref: evaluator.py:340-346].  ``get_all=True``:
    ``(score, precision, recall)`` in sklearn's layout -- every distinct threshold ascending, then the closing point
    (precision 1, recall 0): K + 1 entries, no cut at full recall.  Device tensors: the score is the record's fp64 sum, the
    arrays are ``tp / (tp + fp)`` and ``tp / n_pos`` of the integer curve, finished on the host.  NaN without a positive."""
    if _on_device(pred):
        from .. import ops
        score, label = _dev_score_label(gt, pred)
        counts = ops.rank_counts(score, label)
        rec = _read_record(ops.cls_record(score, label, counts))
        if not get_all:
            return rec["prauc"]
        tp, fp, _ = ops.cls_curve(score, counts, rec["k"])
        precision, recall = _curve_arrays(tp.cpu().numpy(), fp.cpu().numpy(), rec["n_pos"])
        return rec["prauc"], precision, recall
    y, s = _host_score_label(gt, pred)
    tp, fp, _ = _host_curve(y, s)
    precision, recall = _curve_arrays(tp, fp, int(y.sum()))
    area = _trapezoid(precision, recall) if y.any() else _NAN
    return (area, precision, recall) if get_all else area


def binary_metrics(gt, pred, threshold=0.5) -> Dict:
    """One finding's dict with the keys ``classification_score`` consumes plus ``"AP"``: ``AUROC``, ``pF``
    (= ``pfbeta_binarized``), ``prauc``, then ``F1``, ``Accuracy`` and ``ACC_POSITIVES`` (the share of positives predicted
    positive [ref: Classifiers/experiments.py:66-69]) at ``pred >= threshold``, and the average precision ``AP``.  Device
    tensors: one counts pass, one reduction, and one read of the 20-slot record -- no per-sample data leaves the device."""
    if _on_device(pred):
        from .. import ops
        score, label = _dev_score_label(gt, pred)
        return _metrics_of_record(_read_record(ops.cls_record(score, label, ops.rank_counts(score, label), threshold)))
    y, s = _host_score_label(gt, pred)
    tp, fp, _ = _host_curve(y, s)
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    precision, recall = _curve_arrays(tp, fp, n_pos)
    hit = s >= threshold
    ctp, cfp = int((hit & y).sum()), int((hit & ~y).sum())
    return _finish_metrics(_host_auroc(y, s), _host_best_pf1(y, s), _trapezoid(precision, recall) if n_pos else _NAN,
                           -float(np.sum(np.diff(recall) * precision[:-1])) if n_pos else _NAN,
                           ctp, cfp, n_neg - cfp, n_pos - ctp)


# ------------------------------------------------------------------------------------------ bootstrap confidence intervals
# The specification is in the module docstring.  Device tensors: csrc/retrieval.hip (mc_boot_records);
# numpy arrays: host Philox, np.bincount, cumsum -- the same records, integer for integer.
BOOT_STREAM = 0x626F6F74          # counter word 2 of every draw
BOOT_MAX_N = 1 << 24
_BOOT_BLOCK_WORDS = 1 << 22       # draws generated at once on the host path


def bootstrap_indices(gt, n_boot, seed=0, stratified=False, first=0) -> np.ndarray:
    """int64 [n_boot, N]: the sample every draw of replicates ``first .. first + n_boot`` picks (``gt`` gives N, and the
    classes when ``stratified``).  The draw of the specification, on the host."""
    from ..augment import philox4x32
    y = np.asarray(gt.cpu() if torch.is_tensor(gt) else gt).reshape(-1) != 0
    n, seed = len(y), int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((n + 3) >> 2, dtype=np.uint64)[None, :]
    r = np.arange(first, first + n_boot, dtype=np.uint64)[:, None]
    words = philox4x32(q, r, BOOT_STREAM, 0x5bd1e995, seed & 0xFFFFFFFF, seed >> 32)
    u = np.stack(words, axis=2).reshape(n_boot, -1)[:, :n]                  # word t & 3 of counter t >> 2 at column t
    s32 = np.uint64(32)
    if not stratified:
        return ((u * np.uint64(n)) >> s32).astype(np.int64)
    pos, neg = np.flatnonzero(y), np.flatnonzero(~y)
    idx = np.empty((n_boot, n), dtype=np.int64)
    if len(pos):
        idx[:, :len(pos)] = pos[((u[:, :len(pos)] * np.uint64(len(pos))) >> s32).astype(np.int64)]
    if len(neg):
        idx[:, len(pos):] = neg[((u[:, len(pos):] * np.uint64(len(neg))) >> s32).astype(np.int64)]
    return idx


def _host_boot_records(y, s, n_boot, threshold, seed, stratified) -> np.ndarray:
    """int64 [n_boot, 20]: the records ``ops.boot_records`` returns, from the same bins and the same draws.  The best-pF1
    candidate maximises tp / (tp + fp + n_pos) in fp64: two different such fractions (denominators below 2^26) are more than
    2^-52 apart, so the fp64 order is the exact order; ``argmax`` keeps the first = the highest threshold on equal value."""
    n = len(s)
    bins = np.searchsorted(np.sort(s), s, side="left")                      # samples with a strictly smaller score
    top = n - 1 - bins                                                      # position in descending order
    sd = np.zeros(n, dtype=np.float64)
    sd[top] = s                                                             # (tied samples store the same value)
    pred = sd >= threshold
    clip = np.clip(sd, 0.0, 1.0)
    out = np.zeros((n_boot, 20), dtype=np.int64)
    f64 = out[:, 16:].view(np.float64)
    block = max(1, _BOOT_BLOCK_WORDS // n)
    for r0 in range(0, n_boot, block):
        idx = bootstrap_indices(y, min(block, n_boot - r0), seed, stratified, first=r0)
        for k, row in enumerate(idx):
            yy, tt = y[row], top[row]
            cp, cn = np.bincount(tt[yy], minlength=n), np.bincount(tt[~yy], minlength=n)
            tp1, fp1 = np.cumsum(cp), np.cumsum(cn)
            tp0, fp0 = tp1 - cp, fp1 - cn
            n_pos, n_neg = int(tp1[-1]), int(fp1[-1])
            rec, fr = out[r0 + k], f64[r0 + k]
            rec[0], rec[1], rec[2], rec[3] = n_pos, n_neg, int(np.sum(cn * tp0)), int(np.sum(cp * cn))
            rec[4], rec[5], rec[6] = 0, 0, 0xFF800000                       # no candidate: (0, 0, -inf)
            rec[7], rec[8] = int(cp[pred].sum()), int(cn[pred].sum())
            rec[9], rec[10] = n_neg - rec[8], n_pos - rec[7]
            here = np.flatnonzero(cp + cn)
            rec[11] = len(here)
            fr[0] = fr[1] = _NAN
            fr[2], fr[3] = float(np.sum(clip * cp)), float(np.sum(clip * cn))
            if n_pos == 0:
                continue
            cand = np.flatnonzero(cp)
            j = cand[np.argmax(tp1[cand] / (tp1[cand] + fp1[cand] + np.float64(n_pos)))]
            rec[4], rec[5] = tp1[j], fp1[j]
            rec[6] = int(np.array([sd[j]], dtype=np.float32).view(np.uint32)[0])
            a1, b1, a0, b0 = (v[here].astype(np.float64) for v in (tp1, fp1, tp0, fp0))
            p1 = a1 / (a1 + b1)
            with np.errstate(divide="ignore", invalid="ignore"):
                p0 = np.where(a0 + b0 > 0, a0 / (a0 + b0), 1.0)             # the curve's start: precision 1
            dr = a1 / np.float64(n_pos) - a0 / np.float64(n_pos)
            fr[0], fr[1] = float(np.sum(dr * (p1 + p0) / 2.0)), float(np.sum(dr * p1))
    return out


def _check_boot_args(n_boot, alpha, n=None):
    if int(n_boot) != n_boot or n_boot < 1 or n_boot > 1 << 20:
        raise ValueError(f"bootstrap: n_boot must be an integer in [1, 2^20], got {n_boot}")
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"bootstrap: alpha must lie inside (0, 1), got {alpha}")
    if n is not None and not 1 <= n <= BOOT_MAX_N:
        raise ValueError(f"bootstrap: the number of samples must lie in [1, 2^24], got {n}")


def _boot_summary(value: Dict, records, alpha, get_all) -> Dict:
    """{key: {"value", "lo", "hi", "se", "n_valid"[, "replicates"]}} from the point estimates and the int64 [B, 20] records"""
    reps = [_metrics_of_record(_record_of_raw(row)) for row in records]
    out = {}
    for key in BINARY_KEYS:
        out[key] = _interval(value[key], np.asarray([m[key] for m in reps], dtype=np.float64), alpha, get_all)
    return out


def _interval(value, vals, alpha, get_all) -> Dict:
    n_valid = int(np.count_nonzero(~np.isnan(vals)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                     # all-NaN keys and ddof=1 of one value give NaN
        lo, hi = np.nanquantile(vals, [alpha / 2.0, 1.0 - alpha / 2.0])
        se = np.nanstd(vals, ddof=1)
    res = {"value": value, "lo": float(lo), "hi": float(hi), "se": float(se), "n_valid": n_valid}
    if get_all:
        res["replicates"] = vals
    return res


def _numel(x) -> int:
    return int(x.numel()) if torch.is_tensor(x) else int(np.asarray(x).size)


def bootstrap_metrics(gt, pred, n_boot=1000, threshold=0.5, seed=0, stratified=False, alpha=0.05, get_all=False) -> Dict:
    """Percentile bootstrap of ``binary_metrics``: ``{key: {"value", "lo", "hi", "se", "n_valid"}}`` for the BINARY_KEYS.
    ``value`` is the point estimate (that path runs first and raises its ValueErrors), ``lo`` / ``hi`` the ``alpha / 2`` and
    ``1 - alpha / 2`` quantiles over ``n_boot`` replicates, ``se`` their standard deviation (ddof 1), ``n_valid`` the
    replicates where the key is not NaN (the others are left out of the three).  ``get_all=True`` adds ``"replicates"``, the
    fp64 [n_boot] values.  ``stratified``: every replicate keeps the class counts.  The resamples depend on ``seed`` (and N,
    and the labels when stratified) only.  Device tensors: ``mc_rank_counts`` once, then ``mc_boot_records``; n_boot records
    of 160 bytes are read back.  numpy arrays: the host path of the same specification, record for record."""
    if _numel(gt) != _numel(pred):
        raise ValueError("one label per score, and at least one score")
    _check_boot_args(n_boot, alpha, _numel(pred))
    if _on_device(pred):
        from .. import ops
        score, label = _dev_score_label(gt, pred)
        counts = ops.rank_counts(score, label)
        value = _metrics_of_record(_read_record(ops.cls_record(score, label, counts, threshold)))
        records = ops.boot_records(score, label, counts, n_boot, threshold, seed, stratified).cpu().numpy()
    else:
        value = binary_metrics(gt, pred, threshold)
        y, s = _host_score_label(gt, pred)
        records = _host_boot_records(y, s, int(n_boot), threshold, seed, stratified)
    return _boot_summary(value, records, alpha, get_all)


def bootstrap_compare(gt, pred_a, pred_b, n_boot=1000, threshold=0.5, seed=0, stratified=False, alpha=0.05,
                      get_all=False) -> Dict:
    """Paired bootstrap of two score vectors on the same cases: both are resampled with the same seed, so replicate r holds
    the same cases for both.  ``{key: {"value", "lo", "hi", "se", "n_valid", "p_le_0"}}`` of the difference ``a - b``:
    ``value`` the difference of the point estimates, the interval and ``se`` over the replicates where both are defined
    (``n_valid``), ``p_le_0`` the share of those with ``a - b <= 0`` (NaN without one)."""
    if not _numel(gt) == _numel(pred_a) == _numel(pred_b):
        raise ValueError("one label per score of either vector, and at least one score")
    a = bootstrap_metrics(gt, pred_a, n_boot, threshold, seed, stratified, alpha, get_all=True)
    b = bootstrap_metrics(gt, pred_b, n_boot, threshold, seed, stratified, alpha, get_all=True)
    out = {}
    for key in BINARY_KEYS:
        diff = a[key]["replicates"] - b[key]["replicates"]
        res = _interval(a[key]["value"] - b[key]["value"], diff, alpha, get_all)
        res["p_le_0"] = float(np.count_nonzero(diff <= 0) / res["n_valid"]) if res["n_valid"] else _NAN
        out[key] = res
    return out


def classification_score(result: Dict) -> Dict:
    """Averages the per-finding dicts of ``result`` (``{finding: binary_metrics(...)}``) into the reference's ``"...(Avg)"``
    keys, adds them to ``result`` and returns it [ref: evaluator.py:255-277]"""
    findings = list(result.values())
    for value in findings:
        for k, v in value.items():
            if isinstance(v, np.floating):
                value[k] = float(v)
    for key, name in (("ACC_POSITIVES", "ACC_POSITIVES(Avg)"), ("pF", "pF(Avg)"), ("prauc", "prauc(Avg)"),
                      ("AUROC", "AUROC(Avg)"), ("F1", "F1(Avg)"), ("Accuracy", "Accuracy(Avg)")):
        result[name] = np.mean([value[key] for value in findings])
    log.info("\n".join(f"{k}: {v}" for k, v in result.items()))
    return result


def multiclass_classification(preds, labels, class_list: Sequence) -> Dict:
    """Per-class accuracy of the argmax over one-hot ``labels`` [N, C], then ``Accuracy(Macro)`` and ``Accuracy(Micro)``
    [ref: evaluator.py:280-298].  Device tensors: torch integer ops, one read of the 2 C counts."""
    c = len(class_list)
    if _on_device(preds):
        lab = torch.as_tensor(labels).to(preds.device)
        hit = preds.argmax(dim=1)[:, None] == torch.arange(c, device=preds.device)[None, :]
        lab = lab[:, :c].to(torch.int64)
        both = torch.stack([(lab * hit).sum(dim=0), lab.sum(dim=0)]).cpu().numpy()
        correct, total, n = both[0], both[1], lab.shape[0]
    else:
        preds, lab = np.asarray(preds), np.asarray(labels)
        arg = np.argmax(preds, axis=1)
        total = np.asarray([lab[:, i].sum() for i in range(c)])
        correct = np.asarray([(lab[:, i] * (arg == i)).sum() for i in range(c)])
        n = len(lab)
    with np.errstate(divide="ignore", invalid="ignore"):
        result = {name: float(np.float64(correct[i]) / np.float64(total[i])) for i, name in enumerate(class_list)}
    result["Accuracy(Macro)"] = float(np.mean(list(result.values())))
    result["Accuracy(Micro)"] = float(correct.sum()) / n
    log.info(" / ".join(f"{k}: {v:.3f}" for k, v in result.items()))
    return result


def _pf1(tp: int, fp: int, n_pos: int) -> float:
    """pfbeta(gt, binarized, 1) of the reference on integer counts: c_precision = tp / (tp + fp), c_recall = tp / n_pos"""
    if n_pos == 0:
        return _NAN
    if tp == 0:
        return 0.0
    p, r = tp / (tp + fp), tp / n_pos
    return 2 * (p * r) / (p + r)


def _finish_metrics(auc_roc, pf, prauc, ap, tp, fp, tn, fn) -> Dict:
    return {"AUROC": auc_roc, "pF": pf, "prauc": prauc,
            "F1": 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0,       # sklearn's f1_score (0 when undefined)
            "Accuracy": (tp + tn) / (tp + fp + tn + fn),
            "ACC_POSITIVES": tp / (tp + fn) if tp + fn else _NAN,
            "AP": ap}


def _metrics_of_record(rec: Dict) -> Dict:
    return _finish_metrics(_auroc(rec["gt"], rec["eq"], rec["n_pos"], rec["n_neg"]),
                           _pf1(rec["best_tp"], rec["best_fp"], rec["n_pos"]), rec["prauc"], rec["ap"],
                           rec["tp"], rec["fp"], rec["tn"], rec["fn"])


def _read_record(record) -> Dict:
    """the one host read of a device record (ops.cls_record); raises for what the device counted as unusable input"""
    rec = _record_of_raw(record.cpu().numpy())
    _raise_bad_input(rec["n_nan"], rec["n_bad_label"])
    return rec


def _record_of_raw(raw) -> Dict:
    """int64 [20] (the layout of ops.cls_record) -> the record dict"""
    from .. import ops
    rec = {k: int(v) for k, v in zip(ops.CLS_RECORD_INTS, raw)}
    rec.update({k: float(v) for k, v in zip(ops.CLS_RECORD_F64, raw[16:].view(np.float64))})
    rec["best_threshold"] = float(np.array([raw[6] & 0xffffffff], dtype=np.uint32).view(np.float32)[0])
    return rec


def _raise_bad_input(n_nan: int, n_bad_label: int):
    if n_nan:
        raise ValueError(f"{n_nan} scores are NaN")
    if n_bad_label:
        raise ValueError(f"{n_bad_label} labels are outside {{0, 1}}")


def _dev_score_label(gt, pred):
    """fp32 contiguous [N] scores and int32 [N] labels on pred's device; a label that is not 0 or 1 (in any dtype) becomes 2,
    which the kernels count -- nothing is read back here"""
    score = pred.reshape(-1).to(torch.float32).contiguous()
    y = torch.as_tensor(np.asarray(gt) if not torch.is_tensor(gt) else gt).to(score.device).reshape(-1)
    if y.numel() != score.numel() or score.numel() == 0:
        raise ValueError("one label per score, and at least one score")
    if y.dtype != torch.int32:
        y = torch.where((y == 0) | (y == 1), y.to(torch.int32), torch.full_like(y, 2, dtype=torch.int32))
    return score, y.contiguous()


def _host_score_label(gt, pred):
    """(bool [N] positives, fp64 [N] scores)"""
    y = np.asarray(gt.cpu() if torch.is_tensor(gt) else gt).reshape(-1)
    s = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred, dtype=np.float64).reshape(-1)
    if len(y) != len(s) or len(s) == 0:
        raise ValueError("one label per score, and at least one score")
    _raise_bad_input(int(np.isnan(s).sum()), int(((y != 0) & (y != 1)).sum()))
    return y != 0, s


def _host_curve(y, s):
    """(tp [K], fp [K], threshold [K]): positives / negatives with score >= each distinct score, ascending"""
    pos, neg, thr = np.sort(s[y]), np.sort(s[~y]), np.unique(s)
    return len(pos) - np.searchsorted(pos, thr, side="left"), len(neg) - np.searchsorted(neg, thr, side="left"), thr


def _curve_arrays(tp, fp, n_pos: int):
    """sklearn's (precision, recall) from the integer curve plus the closing point (1, 0)"""
    tp = tp.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision, recall = tp / (tp + fp), tp / np.float64(n_pos)
    return np.append(precision, 1.0), np.append(recall, 0.0)


def _trapezoid(precision, recall) -> float:
    return -float(np.sum(np.diff(recall) * (precision[1:] + precision[:-1]) / 2.0))


def _host_auroc(y, s) -> float:
    pos, neg = s[y], np.sort(s[~y])
    lo, hi = np.searchsorted(neg, pos, side="left"), np.searchsorted(neg, pos, side="right")
    return _auroc(int(lo.sum()), int((hi - lo).sum()), len(pos), len(neg))


def _host_best_pf1(y, s) -> float:
    if not y.any():
        return _NAN
    pos, neg = np.sort(s[y]), np.sort(s[~y])
    thr = np.unique(pos)
    tp, fp = len(pos) - np.searchsorted(pos, thr, side="left"), len(neg) - np.searchsorted(neg, thr, side="left")
    p, r = tp / (tp + fp), tp / len(pos)
    return float(np.max(2 * (p * r) / (p + r)))


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
