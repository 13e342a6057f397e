"""The text-tower row kernels of csrc/bert.hip against fp64, PER ELEMENT: embedding + LayerNorm, dropout + add + LayerNorm, masked
softmax with dropout and erf-GELU, forward and backward, in the padded and the packed form and with the atomic and the
store-and-sum backward endings.  GPU only (`pytest -m gpu`); references, bounds and their derivation: tests/_text_rows_ref.py;
the same yardstick without a device (renditions that must pass, wrong variants that must fail): tests/test_text_rows_ref.py.

Shapes are the smallest that reach each branch: 1 / 5 / 37 rows (one wave, a partial and ten workgroups of 4 waves), hidden sizes of
1, 63, 64, 65, 96 and 128 vectors of 8, softmax rows on the general body (t = 1, 8, 24, 40, 100, 511, and 64 through a score tensor
that is not 16-byte aligned) and on the 8-keys-per-lane body (t = 16, 64, 512), an embedding batch whose batch groups make two trips
(b = 5 > nbw = 4 at t = 512).  Dropout masks are compared bit for bit with the host Philox; sums are taken into prefilled outputs.

Worst observed err / bound per kernel and storage build (MI355X; every figure is printed by its test, run with -s):
    kernel, output                                   bf16     f16
    add_ln          mean                             0.081    0.087
                    rstd                             0.084    0.463
                    y, dx, dres                      0.999    0.995
                    dgamma (atomic = store-and-sum)  0.435    0.440
                    dbeta  (atomic = store-and-sum)  0.191    0.191
    embedding       mean                             0.031    0.031
                    rstd                             0.070    0.070
                    y                                0.999    0.995
                    dword                            0.041    0.035
                    dpos                             0.037    0.036
                    dtype                            0.029    0.027
                    dgamma                           0.169    0.120
                    dbeta                            0.176    0.311
    softmax         probs, probs_drop, dscores       1.000    1.000   (general body and 8-keys-per-lane body alike)
    GELU            forward, backward                1.000    0.999
    fused attention, fully masked sequence: rel err 2.4e-3 (T = 32) and 2.5e-3 (T = 288) of the 1e-2 allowed; f16 3e-4
The padded and the packed form agree to the third digit everywhere.  The 16-bit outputs sit at their bound because the bound IS
their own rounding (half a 16-bit ulp) plus a few fp32 ulps: nothing but the rounding is left over.  The statistics and the sums
sit far inside (a worst-case chain is never met by random roundings); the controls of tests/test_text_rows_ref.py show that the
bounds still see a single-pass variance, one key left out of a row sum, the tanh form of GELU and one dropped row of a sum.
With softmax_fwd_k as it was before this file (running maximum started at -3.4e38, above mc_mask_bias's -FLT_MAX) the fully masked row
of every general-body case of test_softmax_per_element came back NaN on the device, as the fp32 emulation of
test_text_rows_ref.py::test_fully_masked_row_is_uniform predicts; the three 8-keys-per-lane cases passed there too.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402
import _text_rows_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
ST, F32, F64, U = R.ST, R.F32, R.F64, R.U
EPS = 1e-12
SEED, SID = R.SEED, R.SID
assert ST == ops.BF16 and SEED >> 32 and SEED & 0xFFFFFFFF and SID

WORST = {}


def note(name, got, ref, bound):
    """asserts |got - ref| <= bound per element and every element finite; prints and records the worst err / bound"""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got.float()).all(), name + ": non-finite"
    q = R.ratio(got, ref, bound)
    WORST[name] = max(WORST.get(name, 0.0), q)
    print(f"    {name}: err / bound {q:.3f}")
    assert q <= 1.0, (name, q)


@pytest.fixture
def deterministic_off():
    prev = ops.set_deterministic(False)
    yield
    ops.set_deterministic(prev)


def prefill(shape, seed):
    return R.randn(*shape, seed=seed, scale=0.25, shift=0.5, dtype=F32, device=DEV)


def acc_bound(entry, pre):
    """bound of `pre += sum`: the sum's own bound and the rounding of the addition"""
    return R.sum_bound(entry) + 2 * U * (pre.to(F64).abs() + entry[0].abs())


# ------------------------------------------------------------------------------------------------ add + LayerNorm
def add_ln_bwd_raw(dy, x, res, gamma, mean, rstd, p, row_map, det, dgamma, dbeta):
    """the four backward entry points through the C ABI, accumulating into the caller's dgamma / dbeta"""
    rows, h = x.shape
    dx, dres = torch.empty_like(x), torch.empty_like(x)
    name, rm = ("mc_add_ln_bwd", ()) if row_map is None else ("mc_add_ln_rows_bwd", (row_map.data_ptr(),))
    wsa = ()
    if det:
        wr = L.load().mc_add_ln_bwd_ws_rows(rows)
        ws = torch.full((wr, 2, h), float("nan"), dtype=F32, device=DEV)
        name, wsa = name + "_ws", (ws.data_ptr(), wr)
    L.call(name, dy.data_ptr(), x.data_ptr(), res.data_ptr(), *rm, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, h,
           float(p), SEED, SID, dx.data_ptr(), dres.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), *wsa, ops._st())
    torch.cuda.synchronize()
    return dx, dres


LN_INPUTS = [("normal", 0.0), ("offset", 0.0), ("const", 0.0), ("spike", 0.0), ("normal", 0.1), ("normal", 0.5)]


# (one non-zero element per row: at the widest row only)
LN_CASES = [(h, k, p) for h in (8, 504, 512, 520, 768, 1024) for k, p in LN_INPUTS if k != "spike" or h == 1024]


@pytest.mark.parametrize("h,kind,p", LN_CASES, ids=[f"h{h}-{k}-p{p}" for h, k, p in LN_CASES])
def test_add_ln_per_element(h, kind, p, deterministic_off):
    gamma, beta = R.affine(h, 200 + h, device=DEV)
    for rows in (1, 5, 37):
        for packed in (False, True):
            n = rows + 3 if packed else rows                          # packed: three alignment rows (row_map < 0) at the end
            x, res = R.ln_inputs(kind, n, h, 210 + h + rows, device=DEV)
            dy = R.randn(n, h, seed=220 + h + rows, device=DEV)
            if packed:
                drow = torch.arange(n) + torch.arange(n) // 3 * 2     # rows of a padded layout with gaps
                drow[rows:] = -1
                dy[rows:] = 0
                row_map = drow.to(torch.int32).to(DEV)
            else:
                drow, row_map = torch.arange(n), None
            keep = R.rows_keep_scale(drow, h, p, device=DEV) if p else None
            o = R.add_ln_fwd(x, res, gamma, beta, EPS, keep)
            bw = R.ln_bwd(o, dy)
            tag = f"add_ln[{'packed' if packed else 'padded'}]"
            print(f"  rows {rows} h {h} {kind} p {p} {tag}")
            y, mean, rstd = ops.add_ln_fwd(x, res, gamma, beta, EPS, p, SEED, SID, row_map=row_map)
            if kind == "const":                                       # variance exactly 0: every figure is known exactly
                assert torch.equal(mean.double(), o.mean), "mean of a constant row"
                assert torch.equal(y, beta.to(ST).expand(n, h)), "y of a constant row is the rounded beta"
                assert float((rstd.double() - o.rstd).abs().max()) <= 4 * U * float(o.rstd.max())
                continue                                              # (rstd = 1e6: the backward of such a row says nothing)
            note(tag + " mean", mean, o.mean, o.e_mean)
            note(tag + " rstd", rstd, o.rstd, o.e_rstd)
            note(tag + " y", y, o.y, o.e_y)
            for det in (False, True):
                end = "store-and-sum" if det else "atomic"
                # the kernel alone: the reference's statistics, sums into prefilled outputs
                pre_g, pre_b = prefill((h,), 230), prefill((h,), 231)
                dgamma, dbeta = pre_g.clone(), pre_b.clone()
                dx, dres = add_ln_bwd_raw(dy, x, res, gamma, o.mean.to(F32), o.rstd.to(F32), p, row_map, det, dgamma, dbeta)
                note(f"{tag} dx", dx, *bw["dx"])
                note(f"{tag} dres", dres, *bw["dres"])
                note(f"{tag} dgamma {end}", dgamma.double() - pre_g.double(), bw["dgamma"][0], acc_bound(bw["dgamma"], pre_g))
                note(f"{tag} dbeta {end}", dbeta.double() - pre_b.double(), bw["dbeta"][0], acc_bound(bw["dbeta"], pre_b))
                if p:
                    live = dres.float() != 0
                    assert torch.equal((dx.float() == 0)[live], (keep == 0)[live]), "dropout mask of the backward"
                    assert bool((keep[rows:] == 1).all()), "alignment rows are not dropped"
                # forward and backward chained: the kernel's own statistics, through the ops wrapper of that ending
                ops.set_deterministic(det)
                dx2, dres2, dgamma2, dbeta2 = ops.add_ln_bwd(dy, x, res, gamma, mean, rstd, p, SEED, SID, row_map=row_map)
                ops.set_deterministic(False)
                note(f"{tag} dx", dx2, *bw["dx"])
                note(f"{tag} dres", dres2, *bw["dres"])
                note(f"{tag} dgamma {end}", dgamma2, bw["dgamma"][0], R.sum_bound(bw["dgamma"]))
                note(f"{tag} dbeta {end}", dbeta2, bw["dbeta"][0], R.sum_bound(bw["dbeta"]))


# ------------------------------------------------------------------------------------------------ embedding + LayerNorm
def embed_bwd_raw(dy, ids, tt, cs, gamma, mean, rstd, p, pk, det, outs):
    """the four embedding backward entry points through the C ABI, accumulating into the caller's outputs"""
    word, pos, typ = cs["word_d"], cs["pos_d"], cs["typ_d"]
    h = word.shape[1]
    ptrs = tuple(t.data_ptr() for t in outs)
    ttp = None if tt is None else tt.data_ptr()
    head = (dy.data_ptr(), ids.data_ptr(), ttp) + ((pk.cu.data_ptr(),) if pk is not None else ())
    head += (word.data_ptr(), pos.data_ptr(), typ.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    if pk is None:
        b, t = ids.shape
        rows, shape = b * t, (b, t)
    else:
        b, t, rows, shape = pk.b, pk.max_len, pk.real, (pk.b, pk.max_len, pk.t)
    if det:
        sorted_ids, order = ops.token_rows_by_id(ids.reshape(-1)[:rows])
        nfl = L.load().mc_bert_embed_bwd_ws_floats(b, t, h, rows, None)
        ws = torch.full((nfl,), float("nan"), dtype=F32, device=DEV)
        extra = (rows,) if pk is not None else ()
        L.call("mc_bert_embed_bwd_ws" if pk is None else "mc_bert_embed_rows_bwd_ws", *head, *shape, h, *extra, float(p), SEED, SID,
               *ptrs, sorted_ids.data_ptr(), order.data_ptr(), ws.data_ptr(), nfl, ops._st())
    else:
        L.call("mc_bert_embed_bwd" if pk is None else "mc_bert_embed_rows_bwd", *head, *shape, h, float(p), SEED, SID, *ptrs,
               ops._st())
    torch.cuda.synchronize()


EMBED_LENGTHS = {(3, 16): [16, 5, 9], (5, 512): [512, 300, 1, 17, 511], (2, 1): [1, 1]}


@pytest.mark.parametrize("h", [64, 520, 1024])
@pytest.mark.parametrize("b,t", [(3, 16), (5, 512), (2, 1)])
def test_embedding_per_element(b, t, h, deterministic_off):
    vocab = 50
    gamma, beta = R.affine(h, 300 + h, device=DEV)
    if t == 512:
        assert L.load().mc_bert_embed_bwd_ws_floats(b, t, h, b * t, None) == (b * t + 4 * t + 4 * t) * h     # nbw = 4 < b: two trips
    for packed in (False, True):
        for with_tt in (True, False):
            cs = R.embed_case(b, t, h, with_tt, 310 + t, vocab, EMBED_LENGTHS[(b, t)] if packed else None)
            for k in ("word", "pos", "typ"):
                cs[k + "_d"] = cs[k].to(DEV)
            if packed:
                pk = ops.PackedRows(cs["lengths"], t).to(DEV)
                src = pk.src.long()
                ids = cs["ids"].to(DEV).reshape(-1)[src].contiguous()
                tt = cs["tt"].to(DEV).reshape(-1)[src].contiguous() if with_tt else None
                real, n = pk.real, pk.rows
                pos_ids, drow = pk.pos.long()[:real], pk.row_map.long()[:real].cpu()
            else:
                pk = None
                ids = cs["ids"].to(DEV)
                tt = cs["tt"].to(DEV) if with_tt else None
                real = n = b * t
                pos_ids, drow = torch.arange(t, device=DEV).repeat(b), torch.arange(n)
            dy = R.randn(n, h, seed=320 + t + h, device=DEV)
            for p in (0.0, 0.1):
                keep = R.rows_keep_scale(drow, h, p, device=DEV) if p else None
                flat_tt = None if tt is None else tt.reshape(-1)[:real]
                o = R.embed_fwd(ids.reshape(-1)[:real], pos_ids, flat_tt, cs["word_d"], cs["pos_d"], cs["typ_d"], gamma, beta, EPS,
                                keep)
                bw = R.ln_bwd(o, dy[:real])
                tag = f"embed[{'packed' if packed else 'padded'}]"
                print(f"  b {b} t {t} h {h} tt {with_tt} p {p} {tag}")
                y, mean, rstd = ops.bert_embed_fwd(ids, tt, cs["word_d"], cs["pos_d"], cs["typ_d"], gamma, beta, EPS, p, SEED, SID, pk=pk)
                note(tag + " mean", mean[:real], o.mean, o.e_mean)
                note(tag + " rstd", rstd[:real], o.rstd, o.e_rstd)
                note(tag + " y", y[:real], o.y, o.e_y)
                if p:
                    assert torch.equal(y[:real].float() == 0, (keep == 0) | (o.y == 0)), "dropout mask of the embedding"
                    assert bool((y[:real].float() == 0).any())
                if packed and n > real:
                    assert float(y[real:].float().abs().max()) == 0 and float(mean[real:].abs().max()) == 0 == float(rstd[real:].abs().max())
                for det in (False, True):
                    end = "store-and-sum" if det else "atomic"
                    shapes = ((vocab, h), (max(t, 2), h), (2, h), (h,), (h,))
                    pre = [prefill(s, 330 + i) for i, s in enumerate(shapes)]
                    for stats, who in (((o.mean.to(F32), o.rstd.to(F32)), "reference statistics"), ((mean, rstd), "own statistics")):
                        outs = [t_.clone() for t_ in pre]
                        full = [torch.zeros(n, dtype=F32, device=DEV) for _ in range(2)]
                        for f_, s_ in zip(full, stats):
                            f_[:real] = s_[:real]
                        embed_bwd_raw(dy, ids, tt, cs, gamma, full[0], full[1], p, pk, det, outs)
                        for name, got, pr in zip(("dword", "dpos", "dtype", "dgamma", "dbeta"), outs, pre):
                            note(f"{tag} {name} {end}", got.double() - pr.double(), bw[name][0], acc_bound(bw[name], pr))
                        for u in cs["unused"]:                       # an id that no token names: not touched at all
                            assert torch.equal(outs[0][u].view(torch.int32), pre[0][u].view(torch.int32)), (who, u)


# ------------------------------------------------------------------------------------------------ softmax
def unaligned(t):
    """the same fp32 values one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 5, dtype=F32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


SOFTMAX_T = [(1, "general"), (8, "general"), (24, "general"), (40, "general"), (100, "general"), (511, "general"),
             (64, "general, unaligned"), (16, "v8"), (64, "v8"), (512, "v8")]
SOFTMAX_IN = [(1.0, 0.0), (3.0, 0.0), (20.0, 0.0), (1.0, 1e4)]


@pytest.mark.parametrize("t,body", SOFTMAX_T, ids=[f"t{t}-{b.replace(', ', '-')}" for t, b in SOFTMAX_T])
def test_softmax_per_element(t, body):
    un = body.endswith("unaligned")
    tag = "softmax[" + ("general" if body.startswith("general") else "v8") + "]"
    for rows in (1, 5, 33):
        for sd, offset in SOFTMAX_IN:
            s = R.softmax_scores(rows, t, 400 + t + rows, sd=sd, offset=offset, device=DEV)
            s_in = unaligned(s) if un else s
            print(f"  rows {rows} t {t} sd {sd} offset {offset} {tag}")
            pr, bound = R.softmax_fwd(s)
            probs, pd = ops.softmax_fwd(s_in, 0.0, SEED, SID)
            assert pd.data_ptr() == probs.data_ptr()
            note(tag + " probs", probs, pr, bound)
            if rows >= 3:
                masked = (s == R.NEG)
                masked[-1] = False
                assert float(probs.float()[masked].abs().max() if masked.any() else 0.0) == 0.0, "masked keys are exactly 0"
                assert float(probs[-2, t // 2]) == 1.0, "a row with one live key"
                assert float((probs[-1].double() - 1.0 / t).abs().max()) <= float(bound[-1].max()), "a fully masked row is uniform"
            dp = R.randn(rows, t, seed=410 + t, dtype=F32, device=DEV)
            ds, dbound = R.softmax_bwd(probs, dp, 0.125)
            got = ops.softmax_bwd(probs, unaligned(dp) if un else dp, 0.0, SEED, SID, 0.125)
            note(tag + " dscores", got, ds, dbound)
        if t % 8 or un:
            continue
        for p in (0.1, 0.5):
            s = R.softmax_scores(rows, t, 420 + t, sd=1.0, device=DEV)
            pr, bound = R.softmax_fwd(s)
            keep = R.keep_scale(rows, t, p, SEED, SID, device=DEV)
            probs, pd = ops.softmax_fwd(s, p, SEED, SID)
            note(tag + " probs", probs, pr, bound)
            live = probs.float() > 0
            assert torch.equal((pd.float() == 0)[live], (keep == 0)[live]), "dropout mask of the softmax"
            note(tag + " probs_drop", pd, pr * keep, keep * (bound - R.half_ulp16(pr)) + U * (pr * keep) + R.half_ulp16(pr * keep))
            dp = R.randn(rows, t, seed=430 + t, dtype=F32, device=DEV)
            ds, dbound = R.softmax_bwd(probs, dp, 0.125, keep)
            note(tag + " dscores", ops.softmax_bwd(probs, dp, p, SEED, SID, 0.125), ds, dbound)


# ------------------------------------------------------------------------------------------------ GELU
def test_gelu_every_finite_pattern():
    x = R.all_finite_patterns(DEV)
    y, bound = R.gelu_fwd(x)
    note("gelu", ops.gelu_fwd(x), y, bound)
    for dy in (torch.ones_like(x), R.randn(x.numel(), seed=500, device=DEV)):
        dx, dbound = R.gelu_bwd(x, dy)
        note("gelu bwd", ops.gelu_bwd(dy, x), dx, dbound)
    if ST == torch.bfloat16:                                           # x * x overflows fp32 inside gelu_grad_f: still 0 resp. 1
        far = x.float().abs() > 1e20
        got = ops.gelu_bwd(torch.ones_like(x), x).float()
        assert far.any() and torch.equal(got[far], (x.float()[far] > 0).float())


# ------------------------------------------------------------------------------------------------ fused attention
@pytest.mark.parametrize("t,entry", [(32, "resident"), (288, "long")])
def test_fused_attention_fully_masked_sequence(t, entry):
    """the semantics of an empty report across the routes: every key of sequence 1 carries mc_mask_bias's -FLT_MAX, the context of
    each of its queries is the plain mean of V over all keys (what torch's softmax gives), as from the unfused softmax above"""
    b, nh = 2, 2
    H = nh * 64
    qkv = R.randn(b * t, 3 * H, seed=600 + t, scale=1.5, device=DEV)
    mask = torch.ones(b, t, dtype=torch.long, device=DEV)
    mask[0, t - 5:] = 0
    mask[1] = 0
    maskb = ops.mask_bias(mask)
    assert float(maskb[1].max()) == torch.finfo(F32).min
    if entry == "resident":
        assert ops.attn_supported(t, 64)
        ctx, _ = ops.attn_fwd(qkv, maskb, b, t, nh, 0.125, 0.0, 1, 0)
    else:
        assert ops.attn_long_supported(t, 64)
        ctx, _ = ops.attn_long_fwd(qkv, maskb, b, t, nh, 0.125, 0.0, 1, 0)
    x = qkv.double()
    q, k, v = (x[:, i * H:(i + 1) * H].view(b, t, nh, 64).permute(0, 2, 1, 3) for i in range(3))
    sc = q @ k.transpose(-1, -2) * 0.125 + maskb.double()[:, None, None, :]
    ref = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(b, t, H)
    mean_v = v[1].mean(1)                                               # [nh, 64]
    assert float((ref[1] - mean_v.reshape(1, H)).abs().max()) <= 1e-12
    got = ctx.view(b, t, H).double()
    assert torch.isfinite(got).all()
    for i in range(b):                                                 # the bound of test_fused_attention_vs_torch, per sequence
        e = float((got[i] - ref[i]).abs().max() / ref[i].abs().max())
        print(f"    attention {entry} sequence {i}: rel err {e:.3e}")
        assert e <= 1e-2, (entry, i, e)


def test_zz_worst_observed():
    """prints the table of the module docstring (run the module with -s)"""
    for k in sorted(WORST):
        print(f"    {k:44s} {WORST[k]:.3f}")
