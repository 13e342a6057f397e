"""Packed (variable-length) text encoder on the GPU: kernels through the C ABI, the encoder against the fp32 oracle, packed
against padded with dropout on, alignment rows, the model-level loss, and the fall-backs to the padded path.

Tolerances are the ones the project already holds the same quantities to: ``test_fused_attention_vs_torch`` (context 1e-2,
dQ / dK / dV 1.5e-2), ``test_fused_attention_dropout_matches_unfused_kernels`` (same dropout mask: 4e-3 forward, 6e-3
backward) and ``test_bert_T256_vs_oracle`` (hidden 3e-2, eos cosine 0.999, gradient cosine 0.98 / norm ratio 5 %).
Where packed is compared with padded THROUGH the oracle, the packed error may be 1.5 x the padded one: the two paths apply
the same roundings to the same rows and differ only where a smaller M selects another GEMM kernel, i.e. another fp32
accumulation order."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
from mammo_clip_amd.breastclip import util  # noqa: E402
from mammo_clip_amd.breastclip.loss import build_loss  # noqa: E402
from mammo_clip_amd.breastclip.model import build_model, clip as clipmod  # noqa: E402
from mammo_clip_amd.breastclip.model.modules import load_text_encoder  # noqa: E402
from oracle import arch as oarch, bert as obert, clip as oclip, loss as oloss, weights as ow  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16
LOSS_CFG = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
T256_LENS = [256, 8, 100, 255, 129, 17, 1, 33]        # test_bert_T256_vs_oracle's lengths plus a length-1 and a length-33 report
GKEYS = ["text_encoder.encoder.layer.0.attention.self.query.weight", "text_encoder.encoder.layer.0.attention.self.value.weight",
         "text_encoder.encoder.layer.5.attention.output.dense.weight", "text_encoder.encoder.layer.11.intermediate.dense.weight",
         "text_encoder.encoder.layer.11.output.LayerNorm.weight", "text_encoder.embeddings.position_embeddings.weight"]


def rnd(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def relerr(got, ref):
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def check(got, ref, tol, what=""):
    """the metric of tests/test_kernels_gpu.py: max-abs error relative to max|ref|"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got.float()).all(), what + ": non-finite"
    e = relerr(got, ref)
    print(f"{what}: rel err {e:.3e} (bound {tol})")
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol}"


def _cos_rows(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(torch.nn.functional.cosine_similarity(a, b, dim=1).min())


def _cos_flat(a, b):
    a, b = a.detach().reshape(-1).cpu().double(), b.detach().reshape(-1).cpu().double()
    return float((a @ b) / (a.norm() * b.norm() + 1e-300))


def _attn_torch(qkv, dctx, t, nh, keep=None, p=0.0):
    """fp32 BertSelfAttention core of ONE sequence of t tokens on the same 16-bit operands (tests/test_kernels_gpu.py's
    _attn_torch with b = 1 and no masked key)"""
    H = nh * 64
    x = qkv.float().requires_grad_(True)
    q, k, v = (x[:, i * H:(i + 1) * H].view(t, nh, 64).permute(1, 0, 2) for i in range(3))
    pr = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1)
    if keep is not None:
        pr = pr * keep / (1 - p)
    ctx = (pr @ v).permute(1, 0, 2).reshape(t, H)
    ctx.backward(dctx.float())
    return ctx.detach(), x.grad


def _packed(lengths, t0=256):
    return ops.PackedRows(lengths, t0).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. attention vs torch
@pytest.mark.parametrize("lengths,nh", [
    ([1, 7, 31, 32, 33, 129, 255, 256], 2),
    ([1, 7, 31, 32, 33, 129, 255, 256], 12),
    ([256, 8, 100, 255, 129, 17, 1, 33, 64, 200, 3], 12),
    ([5], 2), ([1], 12), ([256], 2), ([33, 33, 33], 2), ([16, 48, 2, 95], 12),
])
def test_varlen_attention_vs_torch(lengths, nh):
    """variable-length fused attention and its backward against fp32 torch, per sequence, on the same operands; rows
    behind the packed matrix are not touched and the alignment rows hold zeros"""
    assert ops.attn_varlen_supported(max(lengths), 64)
    pk = _packed(lengths)
    H, R, GUARD = nh * 64, pk.rows, 8
    qkv = rnd(R, 3 * H, seed=300 + sum(lengths), scale=1.5)
    dctx = rnd(R, H, seed=301 + sum(lengths))
    nan = float("nan")
    ctx = torch.full((R + GUARD, H), nan, dtype=BF, device=DEV)
    lse = torch.full((R + GUARD, nh, 2), nan, dtype=torch.float32, device=DEV)
    dqkv = torch.full((R + GUARD, 3 * H), nan, dtype=BF, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    mammo_clip_amd.lib.call("mc_attn_varlen_fwd", qkv.data_ptr(), pk.cu.data_ptr(), pk.order.data_ptr(), pk.b, pk.max_len, pk.t,
                            R, nh, 0.125, 0.0, 1, 0, ctx.data_ptr(), lse.data_ptr(), st)
    mammo_clip_amd.lib.call("mc_attn_varlen_bwd", qkv.data_ptr(), pk.cu.data_ptr(), pk.order.data_ptr(), dctx.data_ptr(),
                            lse.data_ptr(), pk.b, pk.max_len, pk.t, R, nh, 0.125, 0.0, 1, 0, dqkv.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.isnan(ctx[R:].float()).all() and torch.isnan(dqkv[R:].float()).all() and torch.isnan(lse[R:]).all()
    assert float(ctx[pk.real:R].float().abs().sum()) == 0.0 and float(dqkv[pk.real:R].float().abs().sum()) == 0.0
    refs, drefs, r0 = [], [], 0
    for n in lengths:
        ref, dref = _attn_torch(qkv[r0:r0 + n], dctx[r0:r0 + n], n, nh)
        refs.append(ref)
        drefs.append(dref)
        r0 += n
    ref, dref = torch.cat(refs), torch.cat(drefs)
    check(ctx[:pk.real], ref, 1e-2, f"varlen context {lengths} nh={nh}")
    for i, nm in enumerate("QKV"):
        check(dqkv[:pk.real, i * H:(i + 1) * H], dref[:, i * H:(i + 1) * H], 1.5e-2, f"varlen d{nm} {lengths} nh={nh}")
    # without the launch order array: same result, bit for bit (the order only decides which workgroup starts first)
    ctx2, lse2 = ops.attn_varlen_fwd(qkv, pk, nh, 0.125, 0.0, 1, 0)
    pk.order = None
    ctx3, lse3 = ops.attn_varlen_fwd(qkv, pk, nh, 0.125, 0.0, 1, 0)
    assert torch.equal(ctx2, ctx3) and torch.equal(ctx2, ctx[:R]) and torch.equal(lse2[:pk.real], lse3[:pk.real])


def test_varlen_attention_rejects_unsupported_shapes():
    assert not ops.attn_varlen_supported(257, 64) and not ops.attn_varlen_supported(0, 64) and not ops.attn_varlen_supported(64, 32)
    pk = _packed([5, 3], 8)
    qkv = rnd(pk.rows, 3 * 64, seed=1)
    pk.max_len = 300
    with pytest.raises(mammo_clip_amd.lib.MammoClipHipError):
        ops.attn_varlen_fwd(qkv, pk, 1, 0.125, 0.0, 1, 0)


# ------------------------------------------------------------------------------------------------ 2. the padded path's dropout
def _padded_and_packed(lengths, T, width, seed, scale=1.0):
    """a padded [b*T, width] matrix with zeros in the padded rows, its packed rows, and the index helpers"""
    b = len(lengths)
    pk = _packed(lengths, T)
    mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).long().to(DEV)
    x = rnd(b * T, width, seed=seed, scale=scale) * mask.view(-1, 1).to(BF)
    real = mask.view(-1).bool()
    xp = torch.zeros((pk.rows, width), dtype=BF, device=DEV)
    xp[:pk.real] = x[real]
    return x, xp, pk, mask, real


@pytest.mark.parametrize("lengths,T,nh", [([256, 8, 100, 255, 129, 17, 1, 33], 256, 12), ([64, 5, 33, 1], 64, 2)])
def test_varlen_attention_drops_what_the_padded_kernel_drops(lengths, T, nh):
    """p = 0.1, one seed: varlen attention on packed rows against mc_attn_fwd / mc_attn_bwd on the padded layout of the same
    data, on the real rows, within the same-mask bounds (another mask would differ by O(1))"""
    b, H, p, seed, sid = len(lengths), nh * 64, 0.1, 1234, 16
    qkv, qkv_p, pk, mask, real = _padded_and_packed(lengths, T, 3 * H, 400 + T, 1.5)
    dctx, dctx_p, *_ = _padded_and_packed(lengths, T, H, 401 + T)
    maskb = ops.mask_bias(mask)
    ctx, lse = ops.attn_fwd(qkv, maskb, b, T, nh, 0.125, p, seed, sid)
    dqkv = ops.attn_bwd(qkv, maskb, dctx, lse, b, T, nh, 0.125, p, seed, sid)
    ctx_p, lse_p = ops.attn_varlen_fwd(qkv_p, pk, nh, 0.125, p, seed, sid)
    dqkv_p = ops.attn_varlen_bwd(qkv_p, pk, dctx_p, lse_p, nh, 0.125, p, seed, sid)
    check(ctx_p[:pk.real], ctx[real], 4e-3, "packed vs padded context (same dropout mask)")
    for i, nm in enumerate("QKV"):
        check(dqkv_p[:pk.real, i * H:(i + 1) * H], dqkv[real][:, i * H:(i + 1) * H], 6e-3, "packed vs padded d" + nm)
    # and the mask really is on: without dropout the context differs by O(1)
    ctx0, _ = ops.attn_varlen_fwd(qkv_p, pk, nh, 0.125, 0.0, seed, sid)
    assert relerr(ctx_p[:pk.real], ctx0[:pk.real]) > 0.05
    # bit-reproducible backward
    assert torch.equal(dqkv_p, ops.attn_varlen_bwd(qkv_p, pk, dctx_p, lse_p, nh, 0.125, p, seed, sid))


def _lengths_past_the_row_caps():
    """40 reports at T = 256 with more than 8192 real tokens, lengths 1 and 256 among them: the padded (10240 rows) and the
    packed layout both leave the first pass of the add+LayerNorm / embedding forward (8192 rows) and run the add+LayerNorm
    backward (2048 rows per pass) five times; the embedding backward takes 8 sequences per round"""
    g = torch.Generator().manual_seed(31)
    lengths = [1, 256] + torch.randint(200, 257, (38,), generator=g).tolist()
    assert len(lengths) == 40 and sum(lengths) > 8192
    return lengths


@pytest.mark.parametrize("lengths,T", [([12, 1, 40, 7, 33], 40), (_lengths_past_the_row_caps(), 256)], ids=["T40", "T256-past-the-caps"])
def test_row_mapped_add_ln_and_embedding_are_bit_exact(lengths, T):
    """per-row arithmetic with the padded layout's dropout indices: against the padded kernels, bit-exact on the real rows"""
    h, p, seed, sid = 768, 0.1, 99, 17
    b = len(lengths)
    x, xp, pk, mask, real = _padded_and_packed(lengths, T, h, 1)
    res, resp, *_ = _padded_and_packed(lengths, T, h, 2)
    dy, dyp, *_ = _padded_and_packed(lengths, T, h, 3)
    gamma, beta = rnd(h, seed=4, dtype=torch.float32) + 1.0, rnd(h, seed=5, dtype=torch.float32)
    y, mean, rstd = ops.add_ln_fwd(x, res, gamma, beta, 1e-12, p, seed, sid)
    yp, meanp, rstdp = ops.add_ln_fwd(xp, resp, gamma, beta, 1e-12, p, seed, sid, row_map=pk.row_map)
    assert torch.equal(yp[:pk.real], y[real]) and torch.equal(meanp[:pk.real], mean[real]) and torch.equal(rstdp[:pk.real], rstd[real])
    assert torch.isfinite(yp.float()).all()
    assert not torch.equal(yp[:pk.real], ops.add_ln_fwd(xp, resp, gamma, beta, 1e-12, 0.0, seed, sid, row_map=pk.row_map)[0][:pk.real])
    dx, dres, dg, db = ops.add_ln_bwd(dy, x, res, gamma, mean, rstd, p, seed, sid)
    dxp, dresp, dgp, dbp = ops.add_ln_bwd(dyp, xp, resp, gamma, meanp, rstdp, p, seed, sid, row_map=pk.row_map)
    assert torch.equal(dxp[:pk.real], dx[real]) and torch.equal(dresp[:pk.real], dres[real])
    assert float(dxp[pk.real:].float().abs().sum()) == 0.0 and float(dresp[pk.real:].float().abs().sum()) == 0.0
    check(dgp, dg, 1e-4, "add_ln dgamma")       # fp32 sums of the same terms (zero rows aside) in another order
    check(dbp, db, 1e-4, "add_ln dbeta")
    # embeddings
    g = torch.Generator().manual_seed(7)
    V = 500
    ids = (torch.randint(1, V, (b, T), generator=g).to(DEV) * mask).contiguous()
    tt = (torch.randint(0, 2, (b, T), generator=g).to(DEV) * mask).contiguous()
    word, pos, typ = (rnd(n, h, seed=10 + i, dtype=torch.float32) for i, n in enumerate((V, max(64, T), 2)))
    ids_p, tt_p = ids.view(-1)[pk.src.long()].contiguous(), tt.view(-1)[pk.src.long()].contiguous()
    e, em, er = ops.bert_embed_fwd(ids, tt, word, pos, typ, gamma, beta, 1e-12, p, seed, 15)
    ep, epm, epr = ops.bert_embed_fwd(ids_p, tt_p, word, pos, typ, gamma, beta, 1e-12, p, seed, 15, pk=pk)
    assert torch.equal(ep[:pk.real], e[real]) and torch.equal(epm[:pk.real], em[real]) and torch.equal(epr[:pk.real], er[real])
    assert float(ep[pk.real:].float().abs().sum()) == 0.0
    ref = ops.bert_embed_bwd(dy, ids, tt, word, pos, typ, gamma, em, er, p, seed, 15)
    got = ops.bert_embed_bwd(dyp, ids_p, tt_p, word, pos, typ, gamma, epm, epr, p, seed, 15, pk=pk)
    for nm, a, r in zip(("dword", "dpos", "dtype", "dgamma", "dbeta"), got, ref):
        check(a, r, 1e-4, "embedding " + nm)     # fp32 atomic sums of identical terms


def test_pool_and_unpack_helpers():
    lengths, T, h = [12, 1, 40, 7, 33], 40, 768
    b = len(lengths)
    x, xp, pk, mask, real = _padded_and_packed(lengths, T, h, 21)
    hid = x.view(b, T, h)
    ln = torch.tensor(lengths, device=DEV)
    assert torch.equal(ops.rows_gather(xp, pk.eos), hid[torch.arange(b), ln - 1].float())
    assert torch.equal(ops.rows_gather(xp, pk.cu[:b]), hid[:, 0].float())
    m = mask.unsqueeze(-1).expand(hid.size()).float()
    mean_ref = torch.sum(hid.float() * m, dim=1) / torch.clamp(m.sum(dim=1), min=1e-9)      # [ref: clip.py:71-75]
    # two fp32 sums of n <= 40 terms in different orders: each within n * 2^-24 = 2.4e-6 of the exact sum, relative to sum|x|
    check(ops.segment_mean_fwd(xp, pk), mean_ref, 1e-5, "segment mean")
    assert torch.equal(ops.unpack_rows(xp, pk, T), x)                        # zeros at the padded positions
    assert torch.equal(ops.pack_rows(x, pk.row_map), xp)
    d = rnd(b, h, seed=22, dtype=torch.float32)
    sc = ops.rows_scatter(d, pk.eos, pk.rows)
    assert torch.equal(sc[pk.eos.long()], d.to(BF)) and float(sc.float().abs().sum()) == float(d.to(BF).float().abs().sum())
    mb = ops.segment_mean_bwd(d, pk)
    ref = (d / ln[:, None].float()).to(BF)[torch.repeat_interleave(torch.arange(b, device=DEV), ln)]
    check(mb[:pk.real], ref, 4e-3, "segment mean backward")          # one 16-bit rounding of the same fp32 quotient
    assert float(mb[pk.real:].float().abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ 3 / 4. encoder vs oracle
def _text_cfg(pooling="eos"):
    return {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
            "gradient_checkpointing": False, "pooling": pooling, "cache_dir": "", "trust_remote_code": True}


def _encoder(dropout):
    te = load_text_encoder(_text_cfg(), vocab_size=28996)
    sd = ow.synth_state_dict(ow.bert_shapes(obert.BertShape(), "text_encoder."), seed=10)
    te.load_state_dict(sd, strict=True)
    te = te.to(DEV)
    if not dropout:
        for lyr in te.text_encoder.encoder.layer:
            lyr.p_attn = lyr.p_hidden = 0.0
        te.text_encoder.config.hidden_dropout_prob = 0.0
    te.train()
    return te, sd


def _tokens(lens, T, seed=3, device=DEV):
    b = len(lens)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 28996, (b, T), generator=g)
    mask = torch.zeros((b, T), dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, 0], ids[i, n - 1] = 101, 102
        ids[i, n:] = 0
        mask[i, :n] = 1
    tok = {"input_ids": ids.to(device), "attention_mask": mask.to(device), "token_type_ids": torch.zeros_like(ids).to(device)}
    return tok, mask.to(DEV), g


@pytest.fixture(scope="module")
def oracle_pair():
    """the setup of test_bert_T256_vs_oracle on T256_LENS, dropout 0, train mode: errors of the padded and of the packed
    encoder against the fp32 oracle (one oracle run)"""
    te, sd = _encoder(dropout=False)
    lens, T = T256_LENS, 256
    b = len(lens)
    tok, mask, g = _tokens(lens, T)
    r = torch.randn((b, T, 768), generator=g).to(DEV) * mask.unsqueeze(-1)
    sdd = {k: v.to(DEV) for k, v in sd.items()}
    sdg = {k: (v.clone().requires_grad_(True) if k in GKEYS else v) for k, v in sdd.items()}
    ref = obert.forward(sdg, tok, obert.BertShape(), prefix="text_encoder.")
    (ref * r).sum().backward()
    ref = ref.detach()
    mk = mask.unsqueeze(-1).bool()
    last = torch.tensor(lens) - 1
    pd = dict(te.named_parameters())
    out = {}
    for mode in ("padded", "packed"):
        te.set_packed(mode == "packed")
        te.zero_grad(set_to_none=True)
        hid = te(tok)
        hid.backward(r.to(hid.dtype))
        rep = {"hidden_relerr": float(((hid.float() - ref) * mk).abs().max() / (ref * mk).abs().max()),
               "eos_cos": _cos_rows(hid.float()[torch.arange(b), last], ref[torch.arange(b), last])}
        for k in GKEYS:
            rep["grad/" + k] = (_cos_flat(pd[k].grad, sdg[k].grad), float(pd[k].grad.norm() / sdg[k].grad.norm()))
        rep["pad_abs_max"] = float((hid.float() * (~mk)).abs().max())
        print("bert T=256", mode, rep)
        out[mode] = rep
    return out


def test_packed_encoder_vs_oracle(oracle_pair):
    """hidden states of the valid tokens, eos embeddings and weight gradients of the PACKED encoder against the fp32 oracle,
    within test_bert_T256_vs_oracle's bounds; padded positions of last_hidden_state are exactly 0"""
    rep = oracle_pair["packed"]
    assert rep["hidden_relerr"] <= 3e-2 and rep["eos_cos"] >= 0.999, rep
    for k in GKEYS:
        assert rep["grad/" + k][0] >= 0.98 and abs(rep["grad/" + k][1] - 1) <= 0.05, (k, rep)
    assert rep["pad_abs_max"] == 0.0, rep


def test_packed_error_vs_oracle_within_1p5x_of_padded(oracle_pair):
    """Both paths apply the same roundings to the same rows; a smaller M may select another GEMM kernel (another fp32
    accumulation order).  Room for that and nothing else: every error of the packed path against the oracle (hidden-state
    relative error, 1 - eos cosine, 1 - gradient cosine) is at most 1.5 x the padded path's."""
    pa, pk = oracle_pair["padded"], oracle_pair["packed"]
    pairs = {"hidden_relerr": (pa["hidden_relerr"], pk["hidden_relerr"]), "1-eos_cos": (1 - pa["eos_cos"], 1 - pk["eos_cos"])}
    for k in GKEYS:
        pairs["1-cos " + k] = (1 - pa["grad/" + k][0], 1 - pk["grad/" + k][0])
    print("error vs oracle (padded, packed):", pairs)
    for name, (e_pad, e_pk) in pairs.items():
        assert e_pk <= 1.5 * e_pad, (name, e_pad, e_pk)


# ------------------------------------------------------------------------------------------------ 4 / 5. packed vs padded
def _tower_run(te, tok, pooling, r, packed):
    """encode_text + backward of one pooling with the call counter reset: the same seeds in both modes"""
    te.set_packed(packed)
    te.text_encoder._calls = 0
    te.zero_grad(set_to_none=True)
    model = types.SimpleNamespace(text_encoder=te, text_pooling=pooling)
    feats = clipmod.BreastClip.encode_text(model, tok)
    feats.backward(r)
    return feats.detach(), {n: p.grad.detach().clone() for n, p in te.named_parameters() if p.grad is not None}


def _assert_same_tower(tag, f_pad, g_pad, f_pk, g_pk):
    assert torch.isfinite(f_pk).all(), tag
    cos = _cos_rows(f_pk, f_pad)
    worst = (1.0, "", 1.0)
    assert g_pad.keys() == g_pk.keys(), (tag, set(g_pad) ^ set(g_pk))
    for n in g_pad:
        assert torch.isfinite(g_pk[n]).all(), (tag, n)
        if float(g_pad[n].norm()) == 0.0:
            assert float(g_pk[n].norm()) == 0.0, (tag, n)
            continue
        c, ratio = _cos_flat(g_pk[n], g_pad[n]), float(g_pk[n].norm() / g_pad[n].norm())
        if c < worst[0]:
            worst = (c, n, ratio)
        assert c >= 0.98 and abs(ratio - 1) <= 0.05, (tag, n, c, ratio)
    print(f"{tag}: pooled cosine {cos:.6f}, worst gradient cosine {worst[0]:.6f} ({worst[1]}, norm ratio {worst[2]:.4f}), "
          f"{len(g_pad)} parameters")
    assert cos >= 0.999, (tag, cos)


@pytest.fixture(scope="module")
def dropout_encoder():
    return _encoder(dropout=True)[0]


@pytest.mark.parametrize("pooling", ["eos", "bos", "mean"])
def test_packed_vs_padded_text_tower_with_dropout(dropout_encoder, pooling):
    """whole text tower, train mode, dropout 0.1, same seed: pooled features (cosine >= 0.999) and ALL parameter gradients
    (cosine >= 0.98, norm ratio within 5 %) of encode_text + backward, packed against padded"""
    te = dropout_encoder
    tok, mask, g = _tokens(T256_LENS, 256)
    r = torch.randn((len(T256_LENS), 768), generator=g).to(DEV)
    f_pad, g_pad = _tower_run(te, tok, pooling, r, packed=False)
    f_pk, g_pk = _tower_run(te, tok, pooling, r, packed=True)
    assert len(g_pad) > 190
    _assert_same_tower("dropout 0.1 / " + pooling, f_pad, g_pad, f_pk, g_pk)
    # the dropout really is on and seeded by the call counter: the next call draws other masks
    te.set_packed(True)
    f_next = clipmod.BreastClip.encode_text(types.SimpleNamespace(text_encoder=te, text_pooling=pooling), tok)
    assert _cos_rows(f_next, f_pk) < 0.9999


def test_alignment_rows_are_inert(dropout_encoder):
    """sum(lengths) = 125 is no multiple of 8: three alignment rows.  The allocator's cache is seeded with NaN before the
    call, so a buffer row that no kernel writes would poison the weight gradients."""
    te = dropout_encoder
    lens, T = [5, 17, 100, 3], 128
    assert sum(lens) % ops.PackedRows.ALIGN
    tok, mask, g = _tokens(lens, T, seed=5)
    r = torch.randn((len(lens), 768), generator=g).to(DEV)
    f_pad, g_pad = _tower_run(te, tok, "eos", r, packed=False)
    for pooling in ("eos", "mean"):
        if pooling != "eos":
            f_pad, g_pad = _tower_run(te, tok, pooling, r, packed=False)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        poison = [torch.full((n,), float("nan"), dtype=torch.float32, device=DEV) for n in (1 << 26, 1 << 24, 1 << 22, 1 << 20, 1 << 18, 1 << 16) for _ in range(4)]
        del poison                                    # back to the caching allocator: the encoder's torch.empty buffers land here
        f_pk, g_pk = _tower_run(te, tok, pooling, r, packed=True)
        _assert_same_tower("alignment rows / " + pooling, f_pad, g_pad, f_pk, g_pk)
    # ... and through last_hidden_state (unpack and its backward)
    te.set_packed(True)
    te.text_encoder._calls = 0
    te.zero_grad(set_to_none=True)
    poison = [torch.full((1 << 24,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(8)]
    del poison
    hid = te(tok)
    assert hid.shape == (len(lens), T, 768) and torch.isfinite(hid.float()).all()
    assert float((hid.float() * (1 - mask).unsqueeze(-1)).abs().max()) == 0.0
    hid.backward(torch.randn(hid.shape, generator=g).to(DEV).to(hid.dtype))
    assert all(torch.isfinite(p.grad).all() for p in te.parameters() if p.grad is not None)


# ------------------------------------------------------------------------------------------------ 6. model level
def _model_cfg(packed):
    cfg = {"name": "clip_custom", "temperature": 0.07,
           "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
           "text_encoder": _text_cfg(), "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
    if packed:
        cfg["text_encoder"]["packed"] = True
    return cfg


def test_model_loss_packed_vs_padded(monkeypatch):
    """BreastClip.forward + the breast_clip loss, B2 + BERT-base, ragged two-report batch, train mode with the stochastic
    layers off.  The padded path's loss deviation from the fp32 oracle is measured first; the packed path gets that
    deviation x 1.5.  One text-encoder call for both reports (2b sequences) and two calls agree in packed mode as in padded
    mode: embeddings cosine >= 0.999, loss within 2e-3 (the smoke test's loss tolerance)."""
    util.GlobalEnv.reset()
    b, T = 4, 32
    arch = oarch.build_arch("efficientnet-b2")
    sd = ow.synth_state_dict(ow.clip_shapes(arch, obert.BertShape()), seed=10)
    batch = ow.synth_batch(b, 64, 64, T, seed=5)
    assert int(batch["text_tokens"]["attention_mask"].sum()) < b * T                  # ragged
    lossf = build_loss(LOSS_CFG)
    bt_dev = {"images": batch["images"].to(DEV), "image_views": batch["image_views"].to(DEV),
              "text_tokens": {k: v.to(DEV) for k, v in batch["text_tokens"].items()},
              "text_tokens2": {k: v.to(DEV) for k, v in batch["text_tokens2"].items()}}
    with torch.backends.cudnn.flags(enabled=False):
        out = oclip.forward({k: v.to(DEV) for k, v in sd.items()}, bt_dev, arch, obert.BertShape(), train=True)
        l_ref = float(oloss.breast_clip_rank(out["image_embeddings"], out["text_embeddings"], out["text_embeddings2"],
                                             out["image_view_embeddings"], out["logit_scale"], 0, b)["loss"])
    res = {}
    for packed in (False, True):
        model = build_model(_model_cfg(packed), LOSS_CFG, types.SimpleNamespace(vocab_size=28996))
        model.load_state_dict(sd, strict=True)
        enc = model.image_encoder
        enc._dropout_p = 0.0
        enc._global_params = enc._global_params._replace(drop_connect_rate=0.0)
        for lyr in model.text_encoder.text_encoder.encoder.layer:
            lyr.p_attn = lyr.p_hidden = 0.0
        model.text_encoder.text_encoder.config.hidden_dropout_prob = 0.0
        model = model.to(DEV).train()
        assert model.text_encoder.packed is packed
        for one_call in (True, False):
            monkeypatch.setattr(clipmod, "_TEXT_ONE_CALL", one_call)
            # host token tensors (the lengths are taken before the copy) in the one-call run, device tensors in the other
            o = model(dict(bt_dev, text_tokens=batch["text_tokens"], text_tokens2=batch["text_tokens2"]) if one_call else bt_dev, DEV)
            loss = lossf(**o, is_train=True)
            total = loss["total"] if isinstance(loss, dict) else loss
            res[(packed, one_call)] = (float(total), o["text_embeddings"].detach(), o["text_embeddings2"].detach())
        total.backward()
        assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
        del model
    dev_pad, dev_pk = abs(res[(False, True)][0] - l_ref), abs(res[(True, True)][0] - l_ref)
    print(f"model loss: oracle {l_ref:.6f}, padded {res[(False, True)][0]:.6f} (|dev| {dev_pad:.3e}), "
          f"packed {res[(True, True)][0]:.6f} (|dev| {dev_pk:.3e})")
    for packed in (False, True):
        one, two = res[(packed, True)], res[(packed, False)]
        print(f"packed={packed}: one call {one[0]:.6f}, two calls {two[0]:.6f}")
        assert abs(one[0] - two[0]) <= 2e-3, (packed, one[0], two[0])
        assert _cos_rows(one[1], two[1]) >= 0.999 and _cos_rows(one[2], two[2]) >= 0.999
    assert _cos_rows(res[(True, True)][1], res[(False, True)][1]) >= 0.999
    assert dev_pk <= 1.5 * dev_pad, (l_ref, dev_pad, dev_pk)


# ------------------------------------------------------------------------------------------------ 7. fall-backs and replays
def test_fallbacks_and_replay(dropout_encoder):
    te = dropout_encoder
    bert = te.text_encoder
    T = 64

    def run(tok, packed, **kw):
        te.set_packed(packed)
        bert._calls = 7
        te.zero_grad(set_to_none=True)
        hid = te(dict(tok, **kw))
        hid.float().square().sum().backward()
        return hid.detach().clone(), bert.encoder.layer[3].intermediate.dense.weight.grad.detach().clone()

    # all masks full: packed on runs the padded launches -- bit-identical output and gradients, dropout on
    tok, _, _ = _tokens([T] * 4, T)
    h0, g0 = run(tok, False)
    h1, g1 = run(tok, True)
    assert torch.equal(h0, h1) and torch.equal(g0, g1) and bert._calls == 8
    # a mask with a hole, and an all-zero row: padded path, bit for bit
    tok, _, _ = _tokens([T, 20, 9, 33], T)
    for edit in ("hole", "empty"):
        tk = {k: v.clone() for k, v in tok.items()}
        if edit == "hole":
            tk["attention_mask"][1, 5] = 0
        else:
            tk["attention_mask"][2] = 0
        h0, g0 = run(tk, False)
        h1, g1 = run(tk, True)
        assert torch.equal(h0, h1) and torch.equal(g0, g1), edit
    # a packed call replayed with the counter restored (the micro-batched engine step) reproduces itself bit for bit, the
    # counter advances by one per call as in the padded path, and host-side lengths give the same call
    h1, g1 = run(tok, True)
    assert bert._calls == 8
    h2, g2 = run(tok, True)
    h3, g3 = run(tok, True, seq_lengths=ops.prefix_lengths(tok["attention_mask"].cpu()))
    assert torch.equal(h1, h2) and torch.equal(g1, g2) and torch.equal(h1, h3) and torch.equal(g1, g3)
    h0, g0 = run(tok, False)
    assert not torch.equal(h0, h1)                                   # the packed launches did run (zeros at the padded positions)
    real = tok["attention_mask"].bool()
    assert _cos_flat(h1[real].float(), h0[real].float()) >= 0.999
    # under no_grad, eval mode, T % 8 != 0
    te.eval()
    try:
        tok5, mask5, _ = _tokens([21, 3, 13], 21)
        with torch.no_grad():
            te.set_packed(False)
            e0 = te(tok5)
            te.set_packed(True)
            e1 = te(tok5)
        assert e1.shape == e0.shape == (3, 21, 768)
        m = mask5.bool()
        assert _cos_flat(e1[m].float(), e0[m].float()) >= 0.999 and float(e1[~m].float().abs().max()) == 0.0
    finally:
        te.train()
        te.set_packed(False)
