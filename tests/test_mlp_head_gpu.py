"""The MLP projection head on the device: kernels, module, model.  GPU only (`pytest -m gpu`).

Reference: everywhere the fp64 restatement of the five formula lines (tests/_mlp_head_common.py, checked against the
reference-generated tests/golden/mlp_head.npz by tests/test_mlp_head.py) with the HOST Philox mask (keep8 of
tests/_attn_exact_cases.py) for the (seed, stream id) the call used, evaluated on the same fp32 operands.  No kernel output
enters a reference, with the one exception the mask test is about: df against the launch's own dz.

Bounds (tests/_mlp_head_common.py: gelu_err, gelu_grad_err, gemm_err, ln_fwd, ln_bwd, module_bounds), per element, from
operation counts: (chain length + a few) * 2^-24 * sum |terms|, the bound of every intermediate carried into its consumers.
  row sums of the row kernels   chain = 8 * (vectors per lane: 1 / 2 / 4) + 6 wave steps + 1
  column sums of the backward   chain = ceil(rows / (4 * workgroups)) + 4 waves + 1 (the fp64 ordered sum rounds once)
  GEMMs                         chain = k + 4 (mc_sgemm: k sequential fmas at most, epilogue)
  z = f k + res                 2 * 2^-24 * (|f k| + |res|): what makes a row with |mean| = 10^4 std hard -- and what a
                                one-pass E[z^2] - mean^2 variance cannot meet (its error is ~ mean^2 * 2^-24 = 6 var there)
  rstd                          the exact interval of (var + eps -+ evar)^-1/2, + 4 roundings
  erff / __expf                 ROCm's installed documentation gives no ulp figure: measured on an MI355X with
                                scripts/device_math_ulp.hip, erff 1.466 ulp, fast __expf 15.827 ulp over the sweep below; the
                                bounds allow twice that
A ratio err / bound above 1 fails.  Worst observed ratios (MI355X, bf16-storage library; every test prints its own, run with -s):
    gelu_fwd 0.502   gelu_bwd_add 0.442
    row kernels: y 0.191  xhat 0.135  rstd 0.120  dz 0.323  df 0.274  dgamma 0.338  dbeta 0.308  dbias 0.120
    rows with |mean| = 10^4 std and constant rows: y 0.101  xhat 0.098  rstd 0.196
    module on the golden operands, eval: dbeta 0.265, the output and the other six gradients <= 0.002;  train, p = 0.1: dbeta 0.155, the rest <= 0.002
    model: embeddings below 5e-4 of a per-element bound of 2.6e-3 (unit vectors of 512); loss |d| 1.0e-6 against a bound of 3.0
The module- and model-level bounds nest worst cases -- a k-term dot product is allowed k roundings in one direction, and its bound
then enters the next dot product through sums of absolute values -- so they grow by two orders of magnitude per stage while the
observed error does not: at the loss the bound says nothing a looser test would not, and the per-element embedding bound (6 % of a
typical element) is the informative model-level check.  The kernel-level bounds are single-stage and tight to a factor 2-10.
"""
import itertools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
import mammo_clip_amd.lib as L  # noqa: E402
from mammo_clip_amd import checkpoint, engine, ops  # noqa: E402
from mammo_clip_amd.breastclip import util  # noqa: E402
from mammo_clip_amd.breastclip.loss import build_loss  # noqa: E402
from mammo_clip_amd.breastclip.model import build_model  # noqa: E402
from mammo_clip_amd.breastclip.model.modules import MLPProjectionHead  # noqa: E402
from mammo_clip_amd.breastclip.optimizer import build_optimizer  # noqa: E402
from oracle import loss as oloss, weights as ow  # noqa: E402

import _mlp_head_common as H  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
SEED, SID = 0xC0FFEE1234567891, 5          # both seed words non-zero
NMAX = int(L.load().mc_mlp_head_max_n())
CAP = int(L.load().mc_mlp_head_ln_bwd_ws_rows(1 << 20))
ROWS = (1, 3, 4, 5, 67, 4 * CAP + 1)        # the last: one row past the backward's capped grid (a second row per wave)
NS = (8, 64, 72, 512, 520, NMAX)
PS = (0.0, 0.1, 0.5)
GUARD = 256                                 # canary floats in front of and behind every kernel output
CANARY = -7.25e11
WORST = {}


def rnd(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(DEV)


def guarded(*shape):
    """(allocation, NaN-prefilled fp32 view) with canaries on both sides of the view"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), CANARY, dtype=F32, device=DEV)
    v = buf[GUARD:GUARD + numel]
    v.fill_(float("nan"))
    assert v.data_ptr() % 16 == 0
    return buf, v.view(*shape)


def intact(buf):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all())


def ratio(name, got, ref_bound):
    ref, bound = ref_bound
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), name
    r = float(((got.double() - ref).abs() / (bound + 1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), r)
    return r


def zeros(t):
    return torch.zeros_like(t)


def raw_fwd(f, res, gamma, beta, p, seed=SEED, sid=SID):
    rows, n = f.shape
    bufs = [guarded(rows, n), guarded(rows, n), guarded(rows)]
    L.call("mc_mlp_head_ln_fwd", f.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), H.EPS, rows, n, p, seed, sid,
           bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), ops._st())
    assert all(intact(b) for b, _ in bufs)
    return [v for _, v in bufs]


def raw_bwd(dy, xhat, rstd, gamma, p, seed=SEED, sid=SID):
    rows, n = xhat.shape
    ws_rows = int(L.load().mc_mlp_head_ln_bwd_ws_rows(rows))
    bufs = [guarded(rows, n), guarded(rows, n), guarded(ws_rows, 3, n), guarded(3, n)]
    L.call("mc_mlp_head_ln_bwd", dy.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), rows, n, p, seed, sid,
           bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), ws_rows, ops._st())
    assert bool(torch.isfinite(bufs[2][1]).all()), "a workspace element was not written"
    L.call("mc_ordered_sum", bufs[2][1].data_ptr(), ws_rows, 3 * n, 3 * n, bufs[3][1].data_ptr(), 0, ops._st())
    assert all(intact(b) for b, _ in bufs)
    return bufs[0][1], bufs[1][1], bufs[3][1], ws_rows


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("count", [1, 3, 4, 1027, 4099])
def test_gelu_kernels(count):
    x = torch.cat([torch.linspace(-6.3, 6.3, count, dtype=F64).float().to(DEV)[: (count + 1) // 2],
                   rnd(count - (count + 1) // 2, seed=count, scale=1.5)])
    dg, add = rnd(count, seed=count + 1), rnd(count, seed=count + 2, scale=0.5)
    x64, dg64, add64 = x.double(), dg.double(), add.double()
    r1 = ratio("gelu_fwd", ops.gelu_f32_fwd(x), (H.gelu64(x64), H.gelu_err(x64)))
    G = H.gelu_grad64(x64)
    bound = dg64.abs() * H.gelu_grad_err(x64) + 2 * H.U * ((dg64 * G).abs() + add64.abs())
    r2 = ratio("gelu_bwd_add", ops.gelu_f32_bwd_add(dg, x, add), (dg64 * G + add64, bound))
    print(f"gelu count {count}: err / bound fwd {r1:.3f} bwd_add {r2:.3f}")
    assert r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("n", NS)
def test_row_kernels_values_mask_and_workspace(n):
    worst = {}
    for (rows, p), case in zip(itertools.product(ROWS, PS), itertools.count()):
        s0 = 1000 * n + 10 * case
        f, res = rnd(rows, n, seed=s0), rnd(rows, n, seed=s0 + 1, shift=0.5)
        gamma, beta = rnd(n, seed=s0 + 2, scale=0.25, shift=1.0), rnd(n, seed=s0 + 3, scale=0.2)
        dy = rnd(rows, n, seed=s0 + 4)
        scale = H.keep_scale(rows, n, p, SEED, SID, DEV)
        keep = scale > 0
        g64, b64 = gamma.double(), beta.double()
        y, xhat, rstd = raw_fwd(f, res, gamma, beta, p)
        fw = H.ln_fwd(f.double(), zeros(scale), res.double(), zeros(scale), g64, b64, scale)
        got = {"y": y, "xhat": xhat, "rstd": rstd}
        # the backward is handed the reference's (xhat, rstd) rounded to fp32: its reference is exact in them
        xh, rs = fw["xhat"][0].float(), fw["rstd"][0].float()
        df, dz, sums, ws_rows = raw_bwd(dy, xh, rs, gamma, p)
        bw = H.ln_bwd(dy.double(), xh.double(), zeros(scale), rs.double(), zeros(rs.double()), g64, scale, ws_rows)
        got.update(dz=dz, df=df, dgamma=sums[0], dbeta=sums[1], dbias=sums[2])
        for k, v in got.items():
            r = ratio(k, v, fw[k] if k in fw else bw[k])
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (k, rows, n, p, r)
        # the mask, bit for bit: dropped elements give 0, kept ones the launch's own dz times fp32(1 / (1 - p))
        inv = torch.tensor(float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))), dtype=F32, device=DEV)
        assert bool((df[~keep] == 0).all()) and torch.equal(df[keep], (dz * inv)[keep]), (rows, n, p)
        if p > 0 and rows * n >= 512:
            assert bool((~keep).any()) and bool(keep.any())
        # the tensor-level wrappers launch the same kernels: same bits
        o = ops.mlp_head_ln_fwd(f, res, gamma, beta, H.EPS, p, SEED, SID)
        assert all(torch.equal(a, b) for a, b in zip(o, (y, xhat, rstd)))
        o = ops.mlp_head_ln_bwd(dy, xh, rs, gamma, p, SEED, SID)
        assert all(torch.equal(a, b) for a, b in zip(o, (df, dz, sums[0], sums[1], sums[2])))
    print(f"row kernels n {n}: worst err / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("n", [72, 512, NMAX])
def test_rows_with_a_dominant_mean_and_constant_rows(n):
    rows = 6
    f, res = rnd(rows, n, seed=n), rnd(rows, n, seed=n + 1, scale=0.0)
    res[0] = 1.0e4                       # |mean| = 10^4 std (f has std 1)
    res[1] = -3.0e4
    f[1] *= 3.0
    f[2], res[2] = 0.25, 0.5             # a constant row whose sums are exact in fp32: variance 0 exactly
    f[3], res[3] = 0.1, 0.6              # a constant row whose sums round
    f[4] = 0.0
    res[4] = 1.0e4                       # constant and large
    gamma, beta = rnd(n, seed=n + 2, scale=0.25, shift=1.0), rnd(n, seed=n + 3, scale=0.2)
    for p in (0.0, 0.1):
        scale = H.keep_scale(rows, n, p, SEED, SID, DEV)
        y, xhat, rstd = raw_fwd(f, res, gamma, beta, p)
        fw = H.ln_fwd(f.double(), zeros(scale), res.double(), zeros(scale), gamma.double(), beta.double(), scale)
        rs = {k: ratio("extreme_" + k, v, fw[k]) for k, v in (("y", y), ("xhat", xhat), ("rstd", rstd))}
        print(f"extreme rows n {n} p {p}: err / bound {rs}; bound on xhat of the 10^4 row {float(fw['xhat'][1][0].max()):.2e}")
        assert max(rs.values()) <= 1.0, rs
        # the bound still means something on the hard row: a fraction of a unit-variance output, where a one-pass variance is
        # off by several times the variance itself
        assert float(fw["xhat"][1][0].max()) < 0.25
        if p == 0.0:
            for r in (2, 4):             # exact constant rows: xhat = 0, the output is beta, rstd = 1 / sqrt(eps)
                assert bool((xhat[r] == 0).all()) and torch.equal(y[r], beta)
                assert abs(float(rstd[r]) * H.EPS ** 0.5 - 1.0) <= 4 * H.U


# ------------------------------------------------------------------------------------------------ module
def _head(w32, emb, n, p):
    head = MLPProjectionHead(emb, n, p)
    head.load_state_dict(w32, strict=True)
    return head.to(DEV)


def _module_case(head, x32, cot32, seed=None, sid=0):
    """one forward + backward of sum(out * cot) on the device: the output, the input gradient, the parameter gradients"""
    for prm in head.parameters():
        prm.grad = None
    xg = x32.clone().requires_grad_(True)
    out = head(xg) if seed is None else head(xg, seed=seed, stream_id=sid)
    (out * cot32).sum().backward()
    got = {"out": out.detach(), "x": xg.grad}
    got.update({k: v.grad for k, v in head.named_parameters()})
    return got


def _check_module(tag, got, x32, w32, cot32, scale, ws_rows):
    w64 = {k: v.double().to(DEV) for k, v in w32.items()}
    mb = H.module_bounds(x32.double(), w64, cot32.double(), scale, ws_rows)
    # the explicit fp64 backward of module_bounds against fp64 autograd over the five formula lines
    out64, g64 = H.head64_grads(x32.double(), w64, cot32.double(), scale)
    g64["out"] = out64
    for k, (ref, _) in mb.items():
        assert float((ref - g64[k]).abs().max()) <= 1e-11 * (1.0 + float(g64[k].abs().max())), k
    rs = {k: ratio(tag, got[k], mb[k]) for k in mb}
    print(f"{tag}: err / bound " + " ".join(f"{k} {v:.3f}" for k, v in rs.items()))
    assert set(rs) == {"out", "x"} | set(H.PARAMS) and max(rs.values()) <= 1.0, rs
    return mb


def test_module_eval_against_the_golden_operands():
    x, w, cot, out, grads = H.load_golden()
    x32, cot32 = x.float().to(DEV), cot.float().to(DEV)
    w32 = {k: v.float() for k, v in w.items()}
    head = _head(w32, 40, 24, 0.1).eval()
    got = _module_case(head, x32, cot32)
    mb = _check_module("module_eval", got, x32, w32, cot32, 1.0, 2)
    # the fp32-rounded operands move the fp64 result by input rounding only: the comparison above is anchored to the file
    assert float((mb["out"][0].cpu() - out).abs().max()) <= 1e-5 * float(out.abs().max())
    for k in grads:
        assert float((mb[k][0].cpu() - grads[k]).abs().max()) <= 1e-5 * float(grads[k].abs().max()), k
    assert head.last_seed is None                    # eval(): p = 0, no mask drawn


def test_module_train_mode_against_fp64_with_the_host_mask():
    m, emb, n, p = 6, 40, 24, 0.1
    _, w, _, _, _ = H.load_golden()
    w32 = {k: v.float() for k, v in w.items()}
    x32, cot32 = rnd(m, emb, seed=5), rnd(m, n, seed=6)
    head = _head(w32, emb, n, p).train()
    got = _module_case(head, x32, cot32, seed=77, sid=2)
    seed, sid = head.last_seed
    assert sid == 2 and seed == MLPProjectionHead.rng_seed * 1000003 + 77
    scale = H.keep_scale(m, n, p, seed, sid, DEV)
    assert bool((scale == 0).any())
    _check_module("module_train", got, x32, w32, cot32, scale, 2)
    # without a seed the head counts its own calls: two calls, two masks
    a = head(x32).detach()
    s1 = head.last_seed
    b = head(x32).detach()
    assert head.last_seed != s1 and not torch.equal(a, b)
    # the same seed again: the same bits
    assert torch.equal(head(x32, seed=77, stream_id=2).detach(), got["out"])


def test_module_backward_is_bit_reproducible_and_honours_needs_input_grad():
    m, emb, n, p = 67, 72, 520, 0.1
    g = torch.Generator().manual_seed(3)
    head = MLPProjectionHead(emb, n, p)
    with torch.no_grad():
        head.layer_norm.weight.add_(0.2 * torch.randn(n, generator=g))
        head.layer_norm.bias.add_(0.1 * torch.randn(n, generator=g))
    head = head.to(DEV).train()
    x32, cot32 = rnd(m, emb, seed=8), rnd(m, n, seed=9)
    prev = ops.set_deterministic(False)
    try:
        runs = []
        for flag in (False, False, True, True):
            ops.set_deterministic(flag)
            runs.append(_module_case(head, x32, cot32, seed=5, sid=1))
    finally:
        ops.set_deterministic(prev)
    for r in runs[1:]:
        assert all(torch.equal(r[k], runs[0][k]) for k in runs[0])
    assert all(float(v.abs().max()) > 0 for v in runs[0].values())
    # a frozen head: the input gradient alone, same bits; a non-differentiable input: the parameter gradients alone
    for prm in head.parameters():
        prm.requires_grad_(False)
    fr = _module_case(head, x32, cot32, seed=5, sid=1)
    assert torch.equal(fr["x"], runs[0]["x"]) and all(fr[k] is None for k in H.PARAMS)
    for prm in head.parameters():
        prm.requires_grad_(True).grad = None
    out = head(x32, seed=5, stream_id=1)
    (out * cot32).sum().backward()
    assert all(torch.equal(v.grad, runs[0][k]) for k, v in head.named_parameters())


# ------------------------------------------------------------------------------------------------ model
B, HH, WW, T = 4, 160, 96, 32               # the smallest image / text shape of tests/test_model_gpu.py (e2e_b5_small)
EMB = ("image_embeddings", "text_embeddings", "text_embeddings2", "image_view_embeddings")


@pytest.fixture(scope="module")
def setup():
    model = build_model(H.cfg("mlp"), H.LOSS_CFG, types.SimpleNamespace(vocab_size=28996))
    sd = H.mlp_state_dict()
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    batch = ow.synth_batch(B, HH, WW, T, seed=21)
    bt = {"images": batch["images"].to(DEV), "image_views": batch["image_views"].to(DEV),
          "text_tokens": {k: v.to(DEV) for k, v in batch["text_tokens"].items()},
          "text_tokens2": {k: v.to(DEV) for k, v in batch["text_tokens2"].items()}}
    return model, build_loss(H.LOSS_CFG), sd, bt, batch


def _reset(model, sd):
    """the model back at its loaded state: parameters, buffers, gradients, seed counters"""
    model.load_state_dict(sd, strict=True)
    model.zero_grad(set_to_none=True)
    irng, trng = engine._rng_counters(model)
    irng.calls, trng._calls = 0, 0
    model.image_projection._calls = model.text_projection._calls = 0
    util.GlobalEnv.reset()


def _heads(model):
    return [(f"{h}.{k}", v) for h in ("image_projection", "text_projection")
            for k, v in getattr(model, h).named_parameters()]


def test_model_reforward_after_rewinding_the_counters_is_bit_identical(setup):
    model, lossf, sd, bt, _ = setup
    _reset(model, sd)
    model.train()
    seeds = []
    hooks = [h.register_forward_hook(lambda m, i, o: seeds.append(m.last_seed))
             for h in (model.image_projection, model.text_projection)]
    try:
        irng, trng = engine._rng_counters(model)
        with torch.no_grad():
            before = (irng.calls, trng._calls)
            out1 = model(bt, DEV)
            irng.calls, trng._calls = before                      # what engine._step_micro does before its re-forward
            out2 = model(bt, DEV)
            out3 = model(bt, DEV)                                 # not rewound: the counters went on, other masks
    finally:
        for h in hooks:
            h.remove()
    assert len(seeds) == 12 and seeds[:4] == seeds[4:8] and seeds[8:] != seeds[:4]
    assert all(torch.equal(out1[k], out2[k]) for k in EMB)
    assert not any(torch.equal(out1[k], out3[k]) for k in EMB)
    # the four head calls of one forward drew four different masks
    masks = [H.keep_mask(B, 512, 0.1, s, i) for s, i in seeds[:4]]
    assert sorted(i for _, i in seeds[:4]) == [0, 1, 2, 3]
    assert all(not m.all() for m in masks)
    assert all(not np.array_equal(a, b) for a, b in itertools.combinations(masks, 2))


def test_model_trainer_steps_in_every_mode(setup):
    model, lossf, sd, bt, _ = setup

    def step(micro=1, **kw):
        _reset(model, sd)
        opt = build_optimizer(model, {"name": "adamw", "config": {"lr": 1e-4, "weight_decay": 1e-4}})
        tr = engine.Trainer(model, lossf, opt, None, DEV, **kw)
        out = tr.step(bt, micro_batches=micro)
        assert bool(torch.isfinite(out["total"]).all()), (micro, kw)
        for name, prm in _heads(model):
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0, (name, micro, kw)
            assert not torch.equal(prm.detach().cpu(), sd[name]), (name, micro, kw)           # the update reached it
        return {k: v.detach().clone() for k, v in model.state_dict().items()}

    step()                                                        # full batch
    step(max_grad_norm=1.0)
    step(micro=2, keep_graphs=1)                                  # one micro-batch re-forwarded from rewound counters
    a = step(deterministic=True)
    b = step(deterministic=True)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    model.freeze_bn(True)
    try:
        step()
    finally:
        model.freeze_bn(False)
    model.text_encoder.set_packed(True)
    try:
        step()
    finally:
        model.text_encoder.set_packed(False)


def test_model_loss_against_the_fp64_head_on_the_same_pooled_features(setup):
    model, lossf, sd, bt, _ = setup
    _reset(model, sd)
    model.eval()                                                  # p = 0
    feats = []
    hooks = [h.register_forward_pre_hook(lambda m, i: feats.append((m, i[0].detach().clone())))
             for h in (model.image_projection, model.text_projection)]
    try:
        with torch.no_grad():
            out = model(bt, DEV)
            loss = float(lossf(**out, is_train=False)["total"])
    finally:
        for h in hooks:
            h.remove()
    assert len(feats) == 4                                        # image, text, text2, view (clip.py's order)
    U = H.U
    emb, err = [], []
    for head, x in feats:
        w64 = {k: v.detach().double() for k, v in head.named_parameters()}
        y, ey = H.module_bounds(x.double(), w64, torch.zeros(B, 512, dtype=F64, device=DEV), 1.0, 1, split_k=True)["out"]
        # through the L2 norm (one wave per row: 8 + 6 + 1 adds, a square root, a division per element)
        nrm = y.norm(dim=1, keepdim=True)
        en = (y.abs() * ey).sum(1, keepdim=True) / nrm + 11 * U * nrm
        emb.append(y / nrm)
        err.append(ey / nrm + y.abs() * en / nrm ** 2 + U * (y / nrm).abs())
        print(f"head input max |x| {float(x.abs().max()):.3g}: bound on y {float(ey.max()):.2e} (|y| <= {float(y.abs().max()):.3g}), "
              f"on the embedding {float(err[-1].max()):.2e}")
    img, txt, txt2, view = emb
    s = float(model.logit_scale.detach().exp())
    ref = float(oloss.breast_clip_rank(img, txt, txt2, view, torch.tensor(s, dtype=F64, device=DEV), 0, B)["loss"])
    # logits s u.v: the operands' bounds, a 512-term fp32 dot product, s = exp(logit_scale) in fp32; a row's cross-entropy moves
    # by at most twice the largest logit error; the fast exp / log of the loss kernel: 32 * 2^-24 * (s + log 2B); the loss is a
    # weighted sum of row means with weights 8 * 0.125 + 1.0 + 0.5 = 2.5
    elog = 0.0
    for (u, eu), (v, ev) in itertools.permutations(list(zip(emb, err)), 2):
        e = s * (eu @ v.abs().T + u.abs() @ ev.T + (512 + 6) * U * (u.abs() @ v.abs().T))
        elog = max(elog, float(e.max()))
    bound = 2.5 * (2.0 * elog + 32 * U * (s + np.log(2 * B)))
    WORST["model_loss"] = abs(loss - ref) / bound
    print(f"loss hip {loss:.7f} fp64 head {ref:.7f} |d| {abs(loss - ref):.2e} bound {bound:.2e} (largest logit bound {elog:.2e})")
    assert abs(loss - ref) <= bound
    for k, e, er in zip(EMB, emb, err):
        assert ratio("model_embeddings", out[k], (e, er)) <= 1.0, k


def test_evaluator_and_checkpoint_round_trip(setup, tmp_path):
    from mammo_clip_amd.breastclip.evaluator import Evaluator
    model, lossf, sd, bt, batch = setup
    _reset(model, sd)
    model.eval()
    with torch.no_grad():                                         # the model's own eval-mode embeddings, call by call
        img = model.encode_image_normalized(bt["images"])
        txt = ops.l2norm_fwd(model.text_projection(model.encode_text(bt["text_tokens"])))[0]
    model.train()                                                 # the evaluator switches to eval itself
    path = checkpoint.save_checkpoint(str(tmp_path / "mlp.tar"), model, config={"model": model.model_config, "loss": H.LOSS_CFG})
    ev = Evaluator(ckpt_path=path, tokenizer=types.SimpleNamespace(vocab_size=28996), device=DEV)
    assert isinstance(ev.model.image_projection, MLPProjectionHead) and not ev.model.training
    np.testing.assert_array_equal(ev.encode_image(batch["images"]), img.cpu().numpy())
    np.testing.assert_array_equal(ev.encode_text(batch["text_tokens"]), txt.cpu().numpy())
    fresh = build_model(H.cfg("mlp"), H.LOSS_CFG, types.SimpleNamespace(vocab_size=28996))
    checkpoint.load_checkpoint(path, fresh, strict=True)
    assert all(torch.equal(v.cpu(), fresh.state_dict()[k]) for k, v in model.state_dict().items())


def test_f16_storage_build_one_loss_scaled_step():
    """the f16 storage library in a process of its own (the storage type is fixed when the library is loaded)"""
    env = dict(os.environ, MC_STORAGE="f16")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_mlp_head_f16_worker.py")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("MLP-F16 ")][-1][len("MLP-F16 "):])
    print("f16 mlp head", r)
    assert r["scaler"] == "LossScaler" and r["skipped"] == 0 and r["loss_finite"], r
    assert r["head_params"] == 12 and r["head_grads_finite_nonzero"] == 12 and r["head_params_changed"] == 12, r


def test_zz_worst_ratios_of_this_run():
    print("worst err / bound: " + json.dumps({k: round(v, 3) for k, v in sorted(WORST.items())}))
    assert all(v <= 1.0 for v in WORST.values()), WORST
