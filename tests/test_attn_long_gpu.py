"""Long fused attention (mc_attn_long_* / mc_attn_varlen_long_*: up to 512 keys) on the GPU: against fp32 torch, against the
resident kernels where both apply (T <= 256), against the unfused GEMM + softmax kernels they replace past 256 keys (same
dropout masks), packed against padded, and through a small text encoder.

Bounds are the ones the project holds the same comparisons to at T = 32..256 (tests/test_kernels_gpu.py,
tests/test_text_packed_gpu.py): context 1e-2 and dQ / dK / dV 1.5e-2 against fp32 torch (1.5e-2 / 2e-2 under dropout), 4e-3 /
6e-3 against another kernel path with the same dropout mask, cosine >= 0.999 for an encoder that switches kernel routes."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402
from mammo_clip_amd.breastclip.model.modules.text_encoder import BertConfigLite, BertModelHIP  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16


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


def _attn_inputs(b, t, nh, seed):
    H = nh * 64
    qkv = rnd(b * t, 3 * H, seed=seed, scale=1.5)
    mask = torch.ones(b, t, dtype=torch.long, device=DEV)
    for i in range(b):
        mask[i, t - (i * 7) % (t // 2):] = 0 if (i * 7) % (t // 2) else 1          # ragged report lengths
    maskb = ops.mask_bias(mask)
    dctx = rnd(b * t, H, seed=seed + 1)
    return qkv, mask, maskb, dctx


def _attn_torch(qkv, mask, dctx, b, t, nh, keep=None, p=0.0):
    """fp32 reference of BertSelfAttention's core on the same 16-bit operands (keep = dropout keep mask [b,nh,t,t])."""
    H = nh * 64
    x = qkv.float().requires_grad_(True)
    q, k, v = (x[:, i * H:(i + 1) * H].view(b, t, nh, 64).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * 0.125 + (1 - mask.float())[:, None, None, :] * torch.finfo(torch.float32).min
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep / (1 - p)
    ctx = (pr @ v).permute(0, 2, 1, 3).reshape(b * t, H)
    ctx.backward(dctx.float())
    return ctx.detach(), x.grad


def _long(qkv, maskb, dctx, b, t, nh, p=0.0, seed=1, sid=0):
    ctx, lse = ops.attn_long_fwd(qkv, maskb, b, t, nh, 0.125, p, seed, sid)
    return ctx, lse, ops.attn_long_bwd(qkv, maskb, dctx, lse, b, t, nh, 0.125, p, seed, sid)


def _unfused(qkv, maskb, dctx, b, t, nh, p, seed, sid):
    """the batched GEMM + softmax kernels of _LayerFn's unfused path: ctx, dqkv, probs, pd"""
    H, M, hd = nh * 64, b * t, 64
    scores = torch.empty((b, nh, t, t), dtype=torch.float32, device=DEV)
    ops.gemm(qkv, qkv[:, H:], scores, t, t, hd, 3 * H, 3 * H, t, c_f32=1, batch=b * nh, nb2=nh,
             sA=(t * 3 * H, hd), sB=(t * 3 * H, hd), sC=(nh * t * t, t * t), bias=maskb, bias_stride1=t, alpha=0.125)
    probs, pd = ops.softmax_fwd(scores, p, seed, sid)
    ctx2 = torch.empty((M, H), dtype=BF, device=DEV)
    ops.gemm(pd, qkv[:, 2 * H:], ctx2, t, hd, t, t, 3 * H, H, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * H, hd))
    dpd = torch.empty((b, nh, t, t), dtype=torch.float32, device=DEV)
    ops.gemm(dctx, qkv[:, 2 * H:], dpd, t, t, hd, H, 3 * H, t, c_f32=1, batch=b * nh, nb2=nh,
             sA=(t * H, hd), sB=(t * 3 * H, hd), sC=(nh * t * t, t * t))
    dq2 = torch.empty((M, 3 * H), dtype=BF, device=DEV)
    ops.gemm(pd, dctx, dq2[:, 2 * H:], t, hd, t, t, H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * H, hd), sC=(t * 3 * H, hd))
    ds = ops.softmax_bwd(probs, dpd, p, seed, sid, 0.125)
    ops.gemm(ds, qkv[:, H:], dq2, t, hd, t, t, 3 * H, 3 * H, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * 3 * H, hd))
    ops.gemm(ds, qkv, dq2[:, H:], t, hd, t, t, 3 * H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * 3 * H, hd))
    return ctx2, dq2, probs, pd


# ------------------------------------------------------------------------------------------------ 1. padded vs torch
@pytest.mark.parametrize("b,t,nh", [(2, 288, 2), (2, 512, 2), (3, 480, 2), (2, 512, 12)])
def test_long_attention_vs_torch(b, t, nh):
    """the first shape past the resident cap (one 32-key block in the second chunk), both chunks full, a part-filled second
    chunk, and 12 heads (head stride); ragged lengths; masked keys have exactly zero dK / dV"""
    assert ops.attn_long_supported(t, 64) and not ops.attn_supported(t, 64)
    qkv, mask, maskb, dctx = _attn_inputs(b, t, nh, 300 + t)
    ctx, lse, dqkv = _long(qkv, maskb, dctx, b, t, nh)
    ref, dref = _attn_torch(qkv, mask, dctx, b, t, nh)
    check(ctx, ref, 1e-2, "long attention context")
    H = nh * 64
    for i, nm in enumerate("QKV"):
        check(dqkv[:, i * H:(i + 1) * H], dref[:, i * H:(i + 1) * H], 1.5e-2, "long attention d" + nm)
    dead = (mask == 0).view(-1)
    assert dead.any() and float(dqkv[dead][:, H:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. holes at the chunk seam
@pytest.mark.parametrize("t", [288, 512])
def test_long_attention_mask_with_holes_at_the_chunk_seam(t):
    b, nh = 3, 2
    H = nh * 64
    qkv, dctx = rnd(b * t, 3 * H, seed=500 + t, scale=1.5), rnd(b * t, H, seed=501 + t)
    mask = torch.ones(b, t, dtype=torch.long, device=DEV)
    mask[0, 250:263] = 0                               # across key 256: the last block of chunk 0 and the first of chunk 1
    mask[0, 1:5] = 0
    mask[2, 2::3] = 0                                  # row 1 stays all ones
    mask[2, t - 7:] = 0
    assert bool((mask[:, 0] == 1).all()) and bool((mask[1] == 1).all())
    maskb = ops.mask_bias(mask)
    ctx, lse, dqkv = _long(qkv, maskb, dctx, b, t, nh)
    ref, dref = _attn_torch(qkv, mask, dctx, b, t, nh)
    check(ctx, ref, 1e-2, "long attention context, mask with holes")
    for i, nm in enumerate("QKV"):
        check(dqkv[:, i * H:(i + 1) * H], dref[:, i * H:(i + 1) * H], 1.5e-2, "long attention d%s, mask with holes" % nm)
    dead = (mask == 0).view(-1)
    assert float(dqkv[dead][:, H:].float().abs().max()) == 0.0          # masked keys: exactly zero dK / dV


# ------------------------------------------------------------------------------------------------ 3. long vs resident
@pytest.mark.parametrize("t", [32, 256])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_long_kernels_match_the_resident_kernels(t, p):
    """where both apply: same context, gradients and lse, same masks"""
    b, nh, seed, sid = 2, 2, 1234, 16
    H = nh * 64
    qkv, mask, maskb, dctx = _attn_inputs(b, t, nh, 600 + t)
    ctx, lse, dqkv = _long(qkv, maskb, dctx, b, t, nh, p, seed, sid)
    ctx_r, lse_r = ops.attn_fwd(qkv, maskb, b, t, nh, 0.125, p, seed, sid)
    dqkv_r = ops.attn_bwd(qkv, maskb, dctx, lse_r, b, t, nh, 0.125, p, seed, sid)
    check(ctx, ctx_r, 4e-3, "long vs resident context")
    for i, nm in enumerate("QKV"):
        check(dqkv[:, i * H:(i + 1) * H], dqkv_r[:, i * H:(i + 1) * H], 6e-3, "long vs resident d" + nm)
    assert torch.isfinite(lse).all() and float(((lse - lse_r).abs() / lse_r.abs().clamp_min(1e-30)).max()) <= 1e-5
    if p > 0:
        ctx0, _ = ops.attn_long_fwd(qkv, maskb, b, t, nh, 0.125, 0.0, seed, sid)
        assert relerr(ctx, ctx0) > 0.05                # the mask is on


# ------------------------------------------------------------------------------------------------ 4. dropout vs the unfused kernels
@pytest.mark.parametrize("b,t,nh", [(2, 512, 2), (2, 288, 2)])
def test_long_attention_dropout_matches_unfused_kernels(b, t, nh):
    """same (seed, stream, element) dropout function as mc_softmax_fwd: the long kernels reproduce the unfused batched-GEMM +
    softmax path they replace, mask for mask, forward and backward"""
    H, p, seed, sid = nh * 64, 0.1, 1234, 16
    qkv, mask, maskb, dctx = _attn_inputs(b, t, nh, 400 + t)
    ctx, lse, dqkv = _long(qkv, maskb, dctx, b, t, nh, p, seed, sid)
    ctx2, dq2, probs, pd = _unfused(qkv, maskb, dctx, b, t, nh, p, seed, sid)
    check(ctx, ctx2, 4e-3, "long vs unfused context (same dropout mask)")
    keep = (pd.float() > 0) | (probs.float() == 0)
    ref, dref = _attn_torch(qkv, mask, dctx, b, t, nh, keep=keep.float(), p=p)
    check(ctx, ref, 1.5e-2, "dropout long attention context vs torch")
    for i, nm in enumerate("QKV"):
        check(dqkv[:, i * H:(i + 1) * H], dq2[:, i * H:(i + 1) * H], 6e-3, "long vs unfused d" + nm)
        check(dqkv[:, i * H:(i + 1) * H], dref[:, i * H:(i + 1) * H], 2e-2, "dropout long attention d%s vs torch" % nm)


# ------------------------------------------------------------------------------------------------ 5. packed vs torch
def _attn_torch_seq(qkv, dctx, t, nh):
    """_attn_torch for ONE sequence of t tokens with no masked key"""
    ones = torch.ones(1, t, dtype=torch.long, device=DEV)
    return _attn_torch(qkv, ones, dctx, 1, t, nh)


@pytest.mark.parametrize("lengths", [[257, 511, 512, 1, 33, 288, 300, 256], [512], [257]])
def test_varlen_long_attention_vs_torch(lengths):
    """per sequence against fp32 torch; the rows behind the packed matrix are not touched, the alignment rows hold zeros, and
    the launch order changes no bit"""
    nh = 2
    assert ops.attn_varlen_long_supported(max(lengths), 64) and not ops.attn_varlen_supported(max(lengths), 64)
    pk = ops.PackedRows(lengths, 512).to(DEV)
    H, R, GUARD = nh * 64, pk.rows, 8
    qkv = rnd(R, 3 * H, seed=300 + sum(lengths), scale=1.5)
    dctx = rnd(R, H, seed=301 + sum(lengths))
    nan = float("nan")
    ctx = torch.full((R + GUARD, H), nan, dtype=BF, device=DEV)
    lse = torch.full((R + GUARD, nh, 2), nan, dtype=torch.float32, device=DEV)
    dqkv = torch.full((R + GUARD, 3 * H), nan, dtype=BF, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    L.call("mc_attn_varlen_long_fwd", qkv.data_ptr(), pk.cu.data_ptr(), pk.order.data_ptr(), pk.b, pk.max_len, pk.t, R, nh, 0.125,
           0.0, 1, 0, ctx.data_ptr(), lse.data_ptr(), st)
    L.call("mc_attn_varlen_long_bwd", qkv.data_ptr(), pk.cu.data_ptr(), pk.order.data_ptr(), dctx.data_ptr(),
           lse.data_ptr(), pk.b, pk.max_len, pk.t, R, nh, 0.125, 0.0, 1, 0, dqkv.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.isnan(ctx[R:].float()).all() and torch.isnan(dqkv[R:].float()).all() and torch.isnan(lse[R:]).all()
    assert float(ctx[pk.real:R].float().abs().sum()) == 0.0 and float(dqkv[pk.real:R].float().abs().sum()) == 0.0
    refs, drefs, r0 = [], [], 0
    for n in lengths:
        ref, dref = _attn_torch_seq(qkv[r0:r0 + n], dctx[r0:r0 + n], n, nh)
        refs.append(ref)
        drefs.append(dref)
        r0 += n
    ref, dref = torch.cat(refs), torch.cat(drefs)
    check(ctx[:pk.real], ref, 1e-2, f"varlen long context {lengths}")
    for i, nm in enumerate("QKV"):
        check(dqkv[:pk.real, i * H:(i + 1) * H], dref[:, i * H:(i + 1) * H], 1.5e-2, f"varlen long d{nm} {lengths}")
    # without the launch order array: same result, bit for bit
    ctx2, lse2 = ops.attn_varlen_long_fwd(qkv, pk, nh, 0.125, 0.0, 1, 0)
    dqkv2 = ops.attn_varlen_long_bwd(qkv, pk, dctx, lse2, nh, 0.125, 0.0, 1, 0)
    pk.order = None
    ctx3, lse3 = ops.attn_varlen_long_fwd(qkv, pk, nh, 0.125, 0.0, 1, 0)
    dqkv3 = ops.attn_varlen_long_bwd(qkv, pk, dctx, lse3, nh, 0.125, 0.0, 1, 0)
    assert torch.equal(ctx2, ctx3) and torch.equal(ctx2, ctx[:R]) and torch.equal(lse2[:pk.real], lse3[:pk.real])
    assert torch.equal(dqkv2, dqkv3) and torch.equal(dqkv2, dqkv[:R])


# ------------------------------------------------------------------------------------------------ 6. packed vs padded, 7. bit-reproducible
def _padded_and_packed(lengths, T, width, seed, scale=1.0):
    """a padded [b*T, width] matrix with zeros in the padded rows, its packed rows, and the index helpers"""
    b = len(lengths)
    pk = ops.PackedRows(lengths, T).to(DEV)
    mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).long().to(DEV)
    x = rnd(b * T, width, seed=seed, scale=scale) * mask.view(-1, 1).to(BF)
    real = mask.view(-1).bool()
    xp = torch.zeros((pk.rows, width), dtype=BF, device=DEV)
    xp[:pk.real] = x[real]
    return x, xp, pk, mask, real


def test_varlen_long_attention_drops_what_the_padded_long_kernel_drops():
    """p = 0.1, one seed: the packed long kernels against the padded long kernels on the padded layout of the same data, on the
    real rows, within the same-mask bounds; both backward kernels are bit-reproducible"""
    lengths, T, nh = [512, 8, 300, 257, 129, 1], 512, 2
    b, H, p, seed, sid = len(lengths), nh * 64, 0.1, 1234, 16
    qkv, qkv_p, pk, mask, real = _padded_and_packed(lengths, T, 3 * H, 400 + T, 1.5)
    dctx, dctx_p, *_ = _padded_and_packed(lengths, T, H, 401 + T)
    maskb = ops.mask_bias(mask)
    ctx, lse, dqkv = _long(qkv, maskb, dctx, b, T, nh, p, seed, sid)
    ctx_p, lse_p = ops.attn_varlen_long_fwd(qkv_p, pk, nh, 0.125, p, seed, sid)
    dqkv_p = ops.attn_varlen_long_bwd(qkv_p, pk, dctx_p, lse_p, nh, 0.125, p, seed, sid)
    check(ctx_p[:pk.real], ctx[real], 4e-3, "packed vs padded long context (same dropout mask)")
    for i, nm in enumerate("QKV"):
        check(dqkv_p[:pk.real, i * H:(i + 1) * H], dqkv[real][:, i * H:(i + 1) * H], 6e-3, "packed vs padded long d" + nm)
    ctx0, _ = ops.attn_varlen_long_fwd(qkv_p, pk, nh, 0.125, 0.0, seed, sid)
    assert relerr(ctx_p[:pk.real], ctx0[:pk.real]) > 0.05          # the mask really is on
    assert torch.equal(dqkv_p, ops.attn_varlen_long_bwd(qkv_p, pk, dctx_p, lse_p, nh, 0.125, p, seed, sid))
    assert torch.equal(dqkv, ops.attn_long_bwd(qkv, maskb, dctx, lse, b, T, nh, 0.125, p, seed, sid))


# ------------------------------------------------------------------------------------------------ 8. encoder level
LENS, T_ENC = (320, 270, 40), 320


@pytest.fixture(scope="module")
def small_bert():
    torch.manual_seed(7)
    model = BertModelHIP(BertConfigLite(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512)).to(DEV)
    model.train()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1000, 28996, (len(LENS), T_ENC), generator=g)
    mask = torch.zeros((len(LENS), T_ENC), dtype=torch.long)
    for i, n in enumerate(LENS):
        mask[i, :n] = 1
        ids[i, n:] = 0
    tok = {"input_ids": ids.to(DEV), "attention_mask": mask.to(DEV), "token_type_ids": torch.zeros_like(ids).to(DEV)}
    w = rnd(len(LENS), T_ENC, 128, seed=11, dtype=torch.float32) * mask.to(DEV)[:, :, None]      # the loss reads real tokens only
    return model, tok, mask.to(DEV).bool(), w


def _set_dropout(model, p):
    model.config.hidden_dropout_prob = p
    for lyr in model.encoder.layer:
        lyr.p_attn = lyr.p_hidden = p


def _run(model, tok, w, packed, calls=0):
    """hidden state and parameter gradients of one call; ``calls`` fixes the dropout seed of the call"""
    model.set_packed(packed)
    model._calls = calls
    model.zero_grad(set_to_none=True)
    h = model(**tok)["last_hidden_state"]
    (h.float() * w).sum().backward()
    return h.detach(), {n: p_.grad.detach().clone() for n, p_ in model.named_parameters() if p_.grad is not None}


def _assert_same(tag, real, a, b):
    """hidden rows and every parameter gradient: cosine >= 0.999.  The one exception is a gradient that is mathematically
    ZERO and holds rounding noise in either run: the key bias (softmax does not see a constant added to a row of scores, so
    sum_j dK_j = 0).  It must be noise-sized in both runs, at most 1e-2 of the same layer's query-bias gradient."""
    (ha, ga), (hb, gb) = a, b
    cos = torch.nn.functional.cosine_similarity(ha[real].double(), hb[real].double(), dim=1)
    print(f"{tag}: hidden cosine min {float(cos.min()):.6f}")
    assert float(cos.min()) >= 0.999, tag
    assert ga.keys() == gb.keys() and len(ga) > 20
    worst = (1.0, "")
    for n in ga:
        if n.endswith("attention.self.key.bias"):
            scale = float(gb[n.replace("key.bias", "query.bias")].abs().max())
            assert max(float(ga[n].abs().max()), float(gb[n].abs().max())) <= 1e-2 * scale, (tag, n)
            continue
        c = float(torch.nn.functional.cosine_similarity(ga[n].flatten().double(), gb[n].flatten().double(), dim=0))
        worst = min(worst, (c, n))
        assert c >= 0.999, (tag, n, c)
    print(f"{tag}: worst gradient cosine {worst}")


def test_encoder_long_route_matches_the_unfused_route(small_bert, monkeypatch):
    model, tok, real, w = small_bert
    _set_dropout(model, 0.0)
    monkeypatch.delenv("MC_FUSED_ATTN", raising=False)
    calls = []
    fwd = ops.attn_long_fwd
    monkeypatch.setattr(ops, "attn_long_fwd", lambda *a, **kw: (calls.append(1), fwd(*a, **kw))[1])
    fused = _run(model, tok, w, False)
    assert len(calls) == 2                             # one long forward per layer
    monkeypatch.setenv("MC_FUSED_ATTN", "0")
    unfused = _run(model, tok, w, False)
    assert len(calls) == 2
    _assert_same("long vs unfused", real, fused, unfused)


def test_encoder_packed_past_256_tokens(small_bert, monkeypatch):
    """packed mode with a report of more than 256 tokens runs (it raised before the long kernels) and agrees with padded"""
    model, tok, real, w = small_bert
    _set_dropout(model, 0.0)
    monkeypatch.delenv("MC_FUSED_ATTN", raising=False)
    calls = []
    fwd = ops.attn_varlen_long_fwd
    monkeypatch.setattr(ops, "attn_varlen_long_fwd", lambda *a, **kw: (calls.append(1), fwd(*a, **kw))[1])
    padded = _run(model, tok, w, False)
    packed = _run(model, tok, w, True)
    model.set_packed(False)
    assert len(calls) == 2
    _assert_same("packed vs padded", real, packed, padded)
    assert float(packed[0][~real].float().abs().max()) == 0.0           # zeros at the padded positions


def test_encoder_packed_and_padded_draw_the_same_dropout(small_bert, monkeypatch):
    model, tok, real, w = small_bert
    monkeypatch.delenv("MC_FUSED_ATTN", raising=False)
    _set_dropout(model, 0.1)
    try:
        padded = _run(model, tok, w, False, calls=5)
        packed = _run(model, tok, w, True, calls=5)
        other = _run(model, tok, w, False, calls=6)
    finally:
        model.set_packed(False)
        _set_dropout(model, 0.0)
    _assert_same("packed vs padded, dropout", real, packed, padded)
    cos = torch.nn.functional.cosine_similarity(other[0][real].double(), padded[0][real].double(), dim=1)
    assert float(cos.min()) < 0.999                    # another seed is another mask: the bound above tells them apart
