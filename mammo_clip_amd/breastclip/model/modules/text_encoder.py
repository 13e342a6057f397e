"""BioClinicalBERT text encoder on hand-written gfx950 kernels.

Mirrors ``HuggingfaceTextEncoder`` (reference: model/modules/text_encoder.py:5-49): same constructor
arguments, ``out_dim`` attribute, ``forward(tokens) -> last_hidden_state [b, T, H]`` and the same
``state_dict`` keys as ``transformers.BertModel`` (``text_encoder.embeddings.word_embeddings.weight`` ...
``text_encoder.encoder.layer.{i}.attention.self.query.weight`` ... ``text_encoder.pooler.dense.*``), so
released checkpoints load with ``strict=True``.  The reference delegates the arithmetic to the third-party
``transformers`` package; here it is one autograd Function per encoder layer built from MFMA GEMMs (fused
QKV projection, batched-strided attention matmuls without any transposes) plus wave-per-row LayerNorm /
softmax kernels.  The pooler is a parameter container only (the reference never uses it, text_encoder.py:49).
"""
from typing import Dict

import torch
from torch import nn
import torch.nn.functional as F

from .... import ops

# Bio_ClinicalBERT = BERT-base-cased shape
BERT_BASE = dict(vocab_size=28996, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                 intermediate_size=3072, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12,
                 hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)


class BertConfigLite:
    def __init__(self, **kw):
        cfg = dict(BERT_BASE)
        cfg.update(kw)
        for k, v in cfg.items():
            setattr(self, k, v)


class _EmbedFn(torch.autograd.Function):
    """``pk`` (ops.PackedRows) set: ``ids`` / ``tt`` hold the real tokens in packed order."""

    @staticmethod
    def forward(ctx, word, pos, typ, gamma, beta, ids, tt, pk, eps, p, seed, sid):
        y, mean, rstd = ops.bert_embed_fwd(ids, tt, word, pos, typ, gamma, beta, eps, p, seed, sid, pk=pk)
        ctx.cfg = (pk, p, seed, sid)
        ctx.params = (word, pos, typ, gamma, beta)
        ctx.save_for_backward(word, pos, typ, gamma, ids, tt, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        word, pos, typ, gamma, ids, tt, mean, rstd = ctx.saved_tensors
        pk, p, seed, sid = ctx.cfg
        dword, dpos, dtyp, dgamma, dbeta = ops.bert_embed_bwd(dy.contiguous(), ids, tt, word, pos, typ, gamma, mean, rstd,
                                                              p, seed, sid, pk=pk)
        dword[0].zero_()       # nn.Embedding(padding_idx=0) never accumulates a gradient for the [PAD] row
        return ops.deliver_param_grads(ctx.params, (dword, dpos, dtyp, dgamma, dbeta)) + (None,) * 7


class _UnpackFn(torch.autograd.Function):
    """packed rows [R, H] -> [b*t, H] with zeros at the padded positions; backward: gather of the real rows"""

    @staticmethod
    def forward(ctx, x, pk):
        ctx.pk = pk
        return ops.unpack_rows(x, pk, pk.t)

    @staticmethod
    def backward(ctx, dy):
        return ops.pack_rows(dy.contiguous(), ctx.pk.row_map), None


class _LayerFn(torch.autograd.Function):
    """One BertLayer: self-attention + output LayerNorm + FFN + output LayerNorm, forward and backward.
    ``pk`` (ops.PackedRows) set: ``x`` holds packed rows -- every GEMM / GELU / column sum runs on pk.rows rows, attention
    per sequence on its own length, and the LayerNorm kernels take the dropout indices of the padded layout from pk.row_map."""

    @staticmethod
    def forward(ctx, x, maskb, lyr, b, t, seed, pk, *params):
        att, H, nh = lyr.attention, lyr.hidden, lyr.heads
        hd = H // nh
        M = b * t if pk is None else pk.rows
        pa, ph = (lyr.p_attn, lyr.p_hidden) if lyr.training else (0.0, 0.0)
        sid = 16 * lyr.index
        sq, sk, sv = att.self.query, att.self.key, att.self.value
        # fused QKV operand: [3H, H] bf16 weight image + [3H] fp32 bias, rebuilt only when one of the six parameters
        # changed (version counters: bumped by the optimizer step / load_state_dict), not on every layer call
        ver = tuple(p_._version for p_ in (sq.weight, sk.weight, sv.weight, sq.bias, sk.bias, sv.bias)) + (sq.weight.data_ptr(), bool(lyr.hilo))
        cache = getattr(lyr, "_qkv_cache", None)
        if cache is None or cache[0] != ver or cache[1].device != x.device:
            wqkv = torch.empty((3 * H, H), dtype=ops.BF16, device=x.device)
            ops.cast_bf16(sq.weight, out=wqkv[:H])
            ops.cast_bf16(sk.weight, out=wqkv[H:2 * H])
            ops.cast_bf16(sv.weight, out=wqkv[2 * H:])
            bqkv = torch.cat([sq.bias.detach(), sk.bias.detach(), sv.bias.detach()]).float().contiguous()
            wlo = None
            if lyr.hilo:                                   # low terms of the two-term bf16 split (set_hilo_weights)
                wlo = torch.empty((3 * H, H), dtype=ops.BF16, device=x.device)
                ops.cast_bf16_lo(sq.weight, out=wlo[:H])
                ops.cast_bf16_lo(sk.weight, out=wlo[H:2 * H])
                ops.cast_bf16_lo(sv.weight, out=wlo[2 * H:])
            lyr._qkv_cache = cache = (ver, wqkv, bqkv, wlo)
        _, wqkv, bqkv, wqkv_lo = cache
        hilo = bool(lyr.hilo)

        def lin(inp, w_hi, bias, w_src, w_lo=None):
            """y = inp . W^T + bias; hi + lo operand mode: a second GEMM adds inp . W_lo^T (the weights then carry 16
            mantissa bits instead of 8: forward-only parity option, the backward uses the high terms)"""
            y_ = ops.linear_fwd(inp, w_hi, bias=bias)
            if hilo:
                y_ = ops.linear_fwd(inp, w_lo if w_lo is not None else ops.cast_bf16_lo(w_src), residual=y_)
            return y_
        qkv = lin(x, wqkv, bqkv, None, wqkv_lo)
        long_attn = False      # the long kernels (257..512 keys)
        if pk is not None:
            if ops.attn_varlen_supported(pk.max_len, hd):
                ctxv, lse = ops.attn_varlen_fwd(qkv, pk, nh, hd ** -0.5, pa, seed, sid)
            elif ops.attn_varlen_long_supported(pk.max_len, hd):
                long_attn = True
                ctxv, lse = ops.attn_varlen_long_fwd(qkv, pk, nh, hd ** -0.5, pa, seed, sid)
            else:
                raise RuntimeError(f"packed text encoder: no variable-length attention kernel for head size {hd}, length {pk.max_len}")
            probs = pd = None
        elif ops.attn_supported(t, hd):
            # one kernel: scores, mask, softmax, dropout and context; only (row max, 1/row sum) are kept for backward
            ctxv, lse = ops.attn_fwd(qkv, maskb, b, t, nh, hd ** -0.5, pa, seed, sid)
            probs = pd = None
        elif ops.attn_long_supported(t, hd):
            long_attn = True
            ctxv, lse = ops.attn_long_fwd(qkv, maskb, b, t, nh, hd ** -0.5, pa, seed, sid)
            probs = pd = None
        else:
            lse = None
            scores = torch.empty((b, nh, t, t), dtype=torch.float32, device=x.device)
            ops.gemm(qkv, qkv[:, H:], scores, t, t, hd, 3 * H, 3 * H, t, c_f32=1, batch=b * nh, nb2=nh,
                     sA=(t * 3 * H, hd), sB=(t * 3 * H, hd), sC=(nh * t * t, t * t), bias=maskb, bias_stride1=t,
                     alpha=hd ** -0.5)
            probs, pd = ops.softmax_fwd(scores, pa, seed, sid)
            del scores
            ctxv = torch.empty((M, H), dtype=ops.BF16, device=x.device)
            ops.gemm(pd, qkv[:, 2 * H:], ctxv, t, hd, t, t, 3 * H, H, b_kmajor=1, batch=b * nh, nb2=nh,
                     sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * H, hd))
        wo = ops.cast_bf16(att.output.dense.weight)
        ao = lin(ctxv, wo, att.output.dense.bias, att.output.dense.weight)
        row_map = None if pk is None else pk.row_map
        ln1, ln2 = att.output.LayerNorm, lyr.output.LayerNorm
        a, mean1, rstd1 = ops.add_ln_fwd(ao, x, ln1.weight, ln1.bias, lyr.eps, ph, seed, sid + 1, row_map=row_map)
        wi = ops.cast_bf16(lyr.intermediate.dense.weight)
        h1 = lin(a, wi, lyr.intermediate.dense.bias, lyr.intermediate.dense.weight)
        hg = ops.gelu_fwd(h1)
        w2 = ops.cast_bf16(lyr.output.dense.weight)
        o = lin(hg, w2, lyr.output.dense.bias, lyr.output.dense.weight)
        y, mean2, rstd2 = ops.add_ln_fwd(o, a, ln2.weight, ln2.bias, lyr.eps, ph, seed, sid + 2, row_map=row_map)
        ctx.lyr, ctx.cfg, ctx.pk = lyr, (b, t, seed, pa, ph, sid), pk
        # hg = gelu(h1) is kept for the FFN2 weight gradient (100 MB per layer at 16384 rows: memory is not the constraint
        # of the text side, a recomputing GELU pass per layer and backward was)
        ctx.sv = dict(x=x, qkv=qkv, probs=probs, pd=pd, lse=lse, maskb=maskb, ctxv=ctxv, ao=ao, a=a, h1=h1, hg=hg, o=o, wqkv=wqkv, wo=wo, wi=wi, w2=w2,
                      qkv_ver=ver, long_attn=long_attn,
                      ln1=(mean1, rstd1), ln2=(mean2, rstd2))
        return y

    @staticmethod
    def backward(ctx, dy):
        lyr, sv = ctx.lyr, ctx.sv
        b, t, seed, pa, ph, sid = ctx.cfg
        att, H, nh = lyr.attention, lyr.hidden, lyr.heads
        hd = H // nh
        x, qkv, probs, pd, a = sv["x"], sv["qkv"], sv["probs"], sv["pd"], sv["a"]
        dy = dy.contiguous()
        g = {}
        pk = ctx.pk
        row_map = None if pk is None else pk.row_map
        # y = LN2(dropout(o) + a)
        do, da_res, g["output.LayerNorm.weight"], g["output.LayerNorm.bias"] = ops.add_ln_bwd(
            dy, sv["o"], a, lyr.output.LayerNorm.weight, sv["ln2"][0], sv["ln2"][1], ph, seed, sid + 2, row_map=row_map)
        hg = sv.pop("hg")
        g["output.dense.weight"] = ops.linear_wgrad(do, hg)
        g["output.dense.bias"] = ops.colsum(do)
        dhg = ops.linear_dgrad(do, sv["w2"], w_t=ops.cast_transpose_bf16(lyr.output.dense.weight))
        del hg, do
        dh1 = ops.gelu_bwd(dhg, sv["h1"])
        del dhg
        g["intermediate.dense.weight"] = ops.linear_wgrad(dh1, a)
        g["intermediate.dense.bias"] = ops.colsum(dh1)
        da = ops.linear_dgrad(dh1, sv["wi"], residual=da_res, w_t=ops.cast_transpose_bf16(lyr.intermediate.dense.weight))
        del dh1, da_res
        # a = LN1(dropout(ao) + x)
        dao, dx_res, g["attention.output.LayerNorm.weight"], g["attention.output.LayerNorm.bias"] = ops.add_ln_bwd(
            da, sv["ao"], x, att.output.LayerNorm.weight, sv["ln1"][0], sv["ln1"][1], ph, seed, sid + 1, row_map=row_map)
        g["attention.output.dense.weight"] = ops.linear_wgrad(dao, sv["ctxv"])
        g["attention.output.dense.bias"] = ops.colsum(dao)
        dctx = ops.linear_dgrad(dao, sv["wo"], w_t=ops.cast_transpose_bf16(att.output.dense.weight))
        del dao
        # attention core
        if pk is not None:
            bwd = ops.attn_varlen_long_bwd if sv["long_attn"] else ops.attn_varlen_bwd
            dqkv = bwd(qkv, pk, dctx, sv["lse"], nh, hd ** -0.5, pa, seed, sid)
        elif sv["lse"] is not None:
            bwd = ops.attn_long_bwd if sv["long_attn"] else ops.attn_bwd
            dqkv = bwd(qkv, sv["maskb"], dctx, sv["lse"], b, t, nh, hd ** -0.5, pa, seed, sid)
        else:
            dpd = torch.empty((b, nh, t, t), dtype=torch.float32, device=x.device)
            ops.gemm(dctx, qkv[:, 2 * H:], dpd, t, t, hd, H, 3 * H, t, c_f32=1, batch=b * nh, nb2=nh,
                     sA=(t * H, hd), sB=(t * 3 * H, hd), sC=(nh * t * t, t * t))
            dqkv = torch.empty((b * t, 3 * H), dtype=ops.BF16, device=x.device)
            ops.gemm(pd, dctx, dqkv[:, 2 * H:], t, hd, t, t, H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
                     sA=(nh * t * t, t * t), sB=(t * H, hd), sC=(t * 3 * H, hd))                       # dV = Pd^T dO
            ds = ops.softmax_bwd(probs, dpd, pa, seed, sid, hd ** -0.5)
            del dpd
            ops.gemm(ds, qkv[:, H:], dqkv, t, hd, t, t, 3 * H, 3 * H, b_kmajor=1, batch=b * nh, nb2=nh,
                     sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * 3 * H, hd))                   # dQ = dS K
            ops.gemm(ds, qkv, dqkv[:, H:], t, hd, t, t, 3 * H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
                     sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * 3 * H, hd))                   # dK = dS^T Q
            del ds
        dwqkv = ops.linear_wgrad(dqkv, x)
        dbqkv = ops.colsum(dqkv)
        tc = getattr(lyr, "_qkv_t_cache", None)                      # [in, 3*out] = wqkv^T, rebuilt only when a weight changed
        if tc is None or tc[0] != sv["qkv_ver"] or tc[1].device != x.device:
            wqkv_t = torch.empty((H, 3 * H), dtype=ops.BF16, device=x.device)
            for i, m_ in enumerate((att.self.query, att.self.key, att.self.value)):
                wqkv_t[:, i * H:(i + 1) * H].copy_(ops.cast_transpose_bf16(m_.weight))
            lyr._qkv_t_cache = tc = (sv["qkv_ver"], wqkv_t)
        wqkv_t = tc[1]
        dx = ops.linear_dgrad(dqkv, sv["wqkv"], residual=dx_res, w_t=wqkv_t)
        for i, nm in enumerate(("query", "key", "value")):
            g[f"attention.self.{nm}.weight"] = dwqkv[i * H:(i + 1) * H]
            g[f"attention.self.{nm}.bias"] = dbqkv[i * H:(i + 1) * H]
        ctx.sv = None
        return (dx, None, None, None, None, None, None) + ops.deliver_param_grads(ops.cached_params(lyr), [g[nm] for nm in lyr._param_names])


# ---------------------------------------------------------------------------------------------- containers
class _Self(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H)


class _SelfOutput(nn.Module):
    def __init__(self, H, eps):
        super().__init__()
        self.dense = nn.Linear(H, H)
        self.LayerNorm = nn.LayerNorm(H, eps=eps)


class _Attention(nn.Module):
    def __init__(self, H, eps):
        super().__init__()
        self.self = _Self(H)
        self.output = _SelfOutput(H, eps)


class _Intermediate(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.dense = nn.Linear(H, I)


class _Output(nn.Module):
    def __init__(self, H, I, eps):
        super().__init__()
        self.dense = nn.Linear(I, H)
        self.LayerNorm = nn.LayerNorm(H, eps=eps)


class BertLayerHIP(nn.Module):
    def __init__(self, cfg, index):
        super().__init__()
        H, I = cfg.hidden_size, cfg.intermediate_size
        self.attention = _Attention(H, cfg.layer_norm_eps)
        self.intermediate = _Intermediate(H, I)
        self.output = _Output(H, I, cfg.layer_norm_eps)
        self.hidden, self.heads, self.eps, self.index = H, cfg.num_attention_heads, cfg.layer_norm_eps, index
        self.p_attn, self.p_hidden = cfg.attention_probs_dropout_prob, cfg.hidden_dropout_prob
        self.hilo = False                  # two-term bf16 weight operands in the forward (BertModelHIP.set_hilo_weights)
        self._param_names = [n for n, _ in self.named_parameters()]

    def forward(self, x, maskb, b, t, seed, pk=None):
        return _LayerFn.apply(x, maskb, self, b, t, seed, pk, *ops.cached_params(self))


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        H = cfg.hidden_size
        self.word_embeddings = nn.Embedding(cfg.vocab_size, H, padding_idx=0)
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, H)
        self.token_type_embeddings = nn.Embedding(cfg.type_vocab_size, H)
        self.LayerNorm = nn.LayerNorm(H, eps=cfg.layer_norm_eps)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([BertLayerHIP(cfg, i) for i in range(cfg.num_hidden_layers)])


class _Pooler(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.dense = nn.Linear(H, H)


class BertModelHIP(nn.Module):
    """``transformers.BertModel``-compatible parameter tree; forward returns ``{"last_hidden_state": [b,T,H]}``."""

    supports_gradient_checkpointing = False

    def __init__(self, cfg: BertConfigLite):
        super().__init__()
        self.config = cfg
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.pooler = _Pooler(cfg.hidden_size)
        for m in self.modules():                      # BERT init: N(0, 0.02), zero bias, unit LayerNorm
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, 0.0, 0.02)
                if isinstance(m, nn.Linear):
                    nn.init.zeros_(m.bias)
        self._calls = 0
        self.rng_seed = 0xBE27
        self.packed = False

    def set_packed(self, on: bool = True):
        """Opt-in packed mode: a call whose attention masks are contiguous prefixes (1..10..0, what the tokenizer produces
        with padding="max_length") runs on the real tokens only -- the b reports concatenated into one [sum(len), H] row
        matrix (ops.PackedRows), attention per sequence on its own length (mc_attn_varlen_*; mc_attn_varlen_long_* when a
        report has more than 256 tokens).  BERT couples tokens only through
        attention and a padded key has probability exactly 0, so the real tokens' outputs, the loss and every gradient are
        those of the padded path; dropout draws the padded path's masks (same seeds, element indices of the padded layout).
        ``last_hidden_state`` then holds ZEROS at the padded positions (the padded path, like the reference, leaves
        unspecified finite values there that nothing reads).  A call with a hole in a mask, an all-zero row or only full
        masks runs the padded launches.  Default off."""
        self.packed = bool(on)
        return self

    def _packed_plan(self, attention_mask, seq_lengths, t0, device):
        """ops.PackedRows of this call, or None when it takes the padded path.  ``seq_lengths``: ops.prefix_lengths of the mask
        as a HOST tensor when the caller had the mask on the host (no synchronisation at all); otherwise the lengths are read
        back from the device mask here -- the one device-to-host copy of a packed call."""
        if not self.packed or attention_mask is None:
            return None
        if seq_lengths is None:
            seq_lengths = ops.prefix_lengths(attention_mask)
        lengths = seq_lengths.tolist()
        if len(lengths) != attention_mask.shape[0] or not ops.packable(lengths, t0):
            return None
        return ops.PackedRows(lengths, t0).to(device)

    def set_hilo_weights(self, on: bool = True):
        """Opt-in precision mode of the encoder's linear layers: every weight matrix enters its MFMA GEMM as TWO bf16 operands
        (high term = the usual bf16 image, low term = bf16 of the remainder; ``mc_cast_f32_bf16_lo``), i.e. two GEMMs per
        layer and the weights carried to 2^-17.  Purpose: the eval-mode parity configuration of DESIGN.md (c) -- with plain
        bf16 weight operands the text side alone moves the eval loss of the reference's bn8k fixture by -1.1e-3 (measured on
        the oracle), above north_star's 1e-3; the reference itself runs these GEMMs in fp32 / fp16 autocast
        [ref: trainer.py:271-278].  Forward only: the backward keeps the high terms.  Default off (2x the BERT GEMM time)."""
        for lyr in self.encoder.layer:
            lyr.hilo = bool(on)
        return self

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, seq_lengths=None, return_packed=False, **_):
        """``seq_lengths`` (optional, packed mode): ops.prefix_lengths(attention_mask) taken on the host.  ``return_packed``:
        a call that ran packed returns ``{"packed_rows": [R, H], "packed": ops.PackedRows}`` instead of forming [b, T, H]."""
        if not input_ids.is_cuda:
            raise RuntimeError("mammo_clip_amd.BertModelHIP runs only on a HIP device (no CPU fallback)")
        b, t0 = input_ids.shape
        pk = self._packed_plan(attention_mask, seq_lengths, t0, input_ids.device)
        if pk is not None:
            return self._forward_packed(input_ids, token_type_ids, pk, return_packed)
        t = t0
        if t % 8:
            # the GEMM / softmax kernels want rows of 16 bytes: pad the sequences with masked [PAD] tokens (they are never
            # attended to, their own outputs are dropped below and carry no gradient) -- any report length is accepted,
            # like the reference's BertModel [ref: text_encoder.py:47-49]
            padn = 8 - t % 8
            input_ids = F.pad(input_ids, (0, padn))
            attention_mask = F.pad(attention_mask if attention_mask is not None else torch.ones((b, t0), dtype=input_ids.dtype, device=input_ids.device), (0, padn))
            token_type_ids = F.pad(token_type_ids, (0, padn)) if token_type_ids is not None else None
            t += padn
        self._calls += 1
        seed = self.rng_seed * 1000003 + self._calls
        cfg = self.config
        emb = self.embeddings
        ids = input_ids.contiguous()
        tt = token_type_ids.contiguous() if token_type_ids is not None else None
        mask = attention_mask.contiguous() if attention_mask is not None else torch.ones_like(ids)
        p = cfg.hidden_dropout_prob if self.training else 0.0
        x = _EmbedFn.apply(emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight,
                           emb.LayerNorm.weight, emb.LayerNorm.bias, ids, tt, None, cfg.layer_norm_eps, p, seed, 15)
        maskb = ops.mask_bias(mask)
        for lyr in self.encoder.layer:
            x = lyr(x, maskb, b, t, seed)
        x = x.view(b, t, cfg.hidden_size)
        return {"last_hidden_state": x if t == t0 else x[:, :t0].contiguous()}

    def _forward_packed(self, input_ids, token_type_ids, pk, return_packed):
        self._calls += 1                                   # the padded path's seed sequence
        seed = self.rng_seed * 1000003 + self._calls
        cfg, emb = self.config, self.embeddings
        ids = torch.index_select(input_ids.reshape(-1), 0, pk.src)
        tt = torch.index_select(token_type_ids.reshape(-1), 0, pk.src) if token_type_ids is not None else None
        p = cfg.hidden_dropout_prob if self.training else 0.0
        x = _EmbedFn.apply(emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight,
                           emb.LayerNorm.weight, emb.LayerNorm.bias, ids, tt, pk, cfg.layer_norm_eps, p, seed, 15)
        for lyr in self.encoder.layer:
            x = lyr(x, None, pk.b, pk.t, seed, pk)
        if return_packed:
            return {"packed_rows": x, "packed": pk}
        x = _UnpackFn.apply(x, pk).view(pk.b, pk.t, cfg.hidden_size)
        return {"last_hidden_state": x if pk.t == pk.t0 else x[:, :pk.t0].contiguous()}


class HuggingfaceTextEncoder(nn.Module):
    """[ref: model/modules/text_encoder.py:5-49]"""

    def __init__(self, name: str = "bert-base-uncased", vocab_size: int = None, pretrained: bool = True,
                 gradient_checkpointing: bool = False, cache_dir: str = "~/.cache/huggingface/hub",
                 local_files_only: bool = False, trust_remote_code: bool = False, config: Dict = None):
        super().__init__()
        # The architecture is fixed to the BERT family (the only one the reference's pre-training configs
        # use); weights come from load_state_dict of a reference / HF checkpoint -- nothing is downloaded.
        self.text_encoder = BertModelHIP(BertConfigLite(**(config or {})))
        self.name, self.pretrained = name, pretrained
        self.out_dim = self.text_encoder.config.hidden_size

    @property
    def packed(self):
        return self.text_encoder.packed

    def set_packed(self, on: bool = True):
        """BertModelHIP.set_packed: skip the padded report tokens (default off; config key model.text_encoder.packed)"""
        self.text_encoder.set_packed(on)
        return self

    def forward_packed(self, x):
        """``(rows [R, H], ops.PackedRows)`` when the call ran packed, ``(last_hidden_state, None)`` when it took the padded
        path -- one encoder call either way (BreastClip.encode_text pools straight from the packed rows)."""
        out = self.text_encoder(**x, return_packed=True)
        if "packed" in out:
            return out["packed_rows"], out["packed"]
        return out["last_hidden_state"], None

    def set_hilo_weights(self, on: bool = True):
        self.text_encoder.set_hilo_weights(on)
        return self

    def forward(self, x):
        out = self.text_encoder(**x)
        return out["last_hidden_state"]
