"""Gradient-norm clipping on the device: mc_grad_norm, mc_grads_unscale_norm_dev, mc_grads_scale_dev, mc_adamw_step_clip and
what is built on them (ops.clip_grad_norm_, AdamW.step(grad_coef=), LossScaler.unscale_(clip=), Trainer(max_grad_norm=)).

The common tensor set: sub-vector sizes, the last lane of the vector body (1023 / 1024), a ragged tail (1027), a chunk of
16384 exactly, a second chunk of length 1, three chunks, and 35 small tensors, so that tensor 40 onwards falls into the second
launch of a call (PACK = 40 in optim.hip).  Zero-element tensors sit first, across that launch boundary, and last.  Layouts:
"own" (one allocation each, 16-byte aligned: the kernels' vector path) and "flat" (views that start 4 bytes past a 16-byte
boundary: the scalar path)."""
import math
import types

import pytest
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import engine, lib as L, ops
from mammo_clip_amd.breastclip import util
from mammo_clip_amd.breastclip.loss import build_loss
from mammo_clip_amd.breastclip.model import build_model
from mammo_clip_amd.breastclip.optimizer import AdamW
from oracle import arch as oarch, bert as obert, weights as ow

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = ops.BF16
CHUNK = 16384
SIZES = [1, 3, 4, 5, 1023, 1024, 1027, CHUNK, CHUNK + 1, 2 * CHUNK + 3] + [17 + i for i in range(35)]
LAYOUTS = ("own", "flat")
INF, NAN = float("inf"), float("nan")
EPS = 2.0 ** -23


def _normals(seed, scale=1.0, shapes=SIZES):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(s if isinstance(s, tuple) else (s,), generator=g) * scale for s in shapes]


def _holes(host):
    hole = torch.empty(0)
    return [hole] + host[:39] + [hole] + host[39:] + [hole]


def _place(host, layout):
    if layout == "own":
        out = [torch.empty_like(h, device=DEV).copy_(h) for h in host]
    else:
        offs, off = [], 1
        for h in host:
            offs.append(off)
            off += (h.numel() + 3) // 4 * 4                # the next view starts at 1 (mod 4) again
        flat = torch.zeros(off, device=DEV)
        out = [flat[o:o + h.numel()].view(h.shape) for o, h in zip(offs, host)]
        for o, h in zip(out, host):
            o.copy_(h)
    assert all((t.data_ptr() % 16 == 0) == (layout == "own") for t in out if t.numel())
    return out


def _cat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _table(grad):
    arr = (L.AdamwTensor * max(len(grad), 1))()
    for a, g in zip(arr, grad):
        a.grad, a.numel = g.data_ptr(), g.numel()
    return arr


def _workspace(arr, n):
    """nan-filled, 8 doubles longer than needed: a chunk sum that is never written, or one written past the end, shows"""
    need = L.load().mc_grad_norm_partials(arr, n)
    return need, torch.full((need + 8,), NAN, dtype=torch.float64, device=DEV)


def _norm(grad, max_norm=INF, n=None):
    arr, n = _table(grad), len(grad) if n is None else n
    need, ws = _workspace(arr, n)
    out = torch.full((2,), -7.0, device=DEV)
    L.call("mc_grad_norm", arr, n, ws.data_ptr(), need, max_norm, out.data_ptr(), ops._st())
    assert torch.isnan(ws[need:]).all() and (need == 0 or not torch.isnan(ws[:need]).all())
    return out


def _norm64(grad):
    return torch.sqrt(sum((g.double() ** 2).sum() for g in grad))


def _coef_ref(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s own expression on an fp32 device scalar"""
    return torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ 1. the norm
@pytest.mark.parametrize("layout", LAYOUTS)
def test_grad_norm_vs_fp64(layout):
    """out[0] against sqrt(sum(g.double()**2)) over the same device values, rtol 2^-23, atol 0 -- derived: an fp64 sum of
    n <= 1.4e8 non-negative terms is off by at most n * 2^-53 = 1.6e-8 relative, the square root halves that, the rounding to
    fp32 adds 2^-24.  Gradient scales 1e-3, 1, 1e3, and 1e-25 / 1e25 whose fp32 squares underflow / overflow."""
    for k, scale in enumerate((1e-3, 1.0, 1e3, 1e-25, 1e25)):
        g = _place(_holes(_normals(10 + k, scale)), layout)
        out = _norm(g)
        ref = _norm64(g)
        print(f"norm [{layout}] scale {scale:g}: got {out[0].item():.9g} ref {ref.item():.17g} "
              f"rel {abs(out[0].double() - ref).item() / ref.item():.3g}")
        assert math.isfinite(out[0].item()) and out[0].item() > 0
        assert abs(out[0].double() - ref).item() <= EPS * ref.item(), (scale, out, ref)
        assert out[1].item() == 1.0, scale                        # max_norm = inf
    out = _norm(g, max_norm=1.0, n=0)                             # an empty call
    assert out.tolist() == [0.0, 1.0]
    out = _norm([torch.empty(0, device=DEV)] * 3, max_norm=0.5)   # nothing but empty tensors
    assert out.tolist() == [0.0, 1.0]


def test_grad_norm_more_partials_than_finish_threads():
    """a 300-chunk tensor among the common set: the finish kernel's 256 threads each take more than one partial"""
    host = _holes(_normals(20))
    g = _place(host[:12], "own") + [torch.randn(300 * CHUNK, device=DEV, generator=torch.Generator(device=DEV).manual_seed(21))] \
        + _place(host[12:], "flat")
    assert L.load().mc_grad_norm_partials(_table(g), len(g)) == 300 + 13 + 35 > 256
    out, ref = _norm(g), _norm64(g)
    print(f"norm with 348 partials: got {out[0].item():.9g} ref {ref.item():.17g}")
    assert abs(out[0].double() - ref).item() <= EPS * ref.item()


# ------------------------------------------------------------------------------------------------ 2. the coefficient
@pytest.mark.parametrize("layout", LAYOUTS)
def test_clip_coefficient_is_torchs(layout):
    """out[1] BIT-equal to torch.clamp(max_norm / (norm + 1e-6), max=1.0) evaluated by torch in fp32 on the returned out[0]:
    max_norm well below the norm, well above it, within 1 % on either side, equal to it, and inf (exactly 1).  A nan among
    the gradients gives a nan norm and a nan coefficient, an inf gives an inf norm and coefficient 0, like the expression."""
    for k, scale in enumerate((1e-3, 1.0, 1e3)):
        g = _place(_holes(_normals(30 + k, scale)), layout)
        nrm = _norm(g)[0].item()
        for f in (0.1, 1e-4, 10.0, 0.995, 0.9999, 1.0, 1.0001, 1.005, INF):
            max_norm = _f32(nrm * f)
            out = _norm(g, max_norm)
            want = _coef_ref(out[0], max_norm)
            assert out[0].item() == nrm
            assert torch.equal(_bits(out[1]), _bits(want)), (scale, f, out[1].item(), want.item())
            assert 0.0 < out[1].item() <= 1.0 and (f == 1.0 or (out[1].item() == 1.0) == (f > 1.0)), (scale, f, out)
    assert _norm(g, INF)[1].item() == 1.0
    g[7][1025] = NAN                                              # the ragged tail of the 1027-element tensor
    out = _norm(g, 2.0)
    assert math.isnan(out[0].item()) and math.isnan(out[1].item()) and math.isnan(_coef_ref(out[0], 2.0).item()), out
    g[7][1025] = INF
    out = _norm(g, 2.0)
    assert out[0].item() == INF and torch.equal(_bits(out[1]), _bits(_coef_ref(out[0], 2.0))) and out[1].item() == 0.0, out


# ------------------------------------------------------------------------------------------------ 3. reproducibility
@pytest.mark.parametrize("layout", LAYOUTS)
def test_grad_norm_is_reproducible_and_fused_unscale_is_the_sequence(layout):
    """three repeats and a run on a second stream give bit-equal [norm, coefficient]; mc_grads_unscale_norm_dev stores the
    gradients mc_grads_unscale_dev stores and returns what mc_grad_norm returns after it, bit for bit (scale 2^16: exact
    products; 3000: rounded ones), flag 0; with an inf in one gradient both set the flag and agree on a non-finite norm."""
    host = _holes(_normals(40))
    g = _place(host, layout)
    first = _norm(g, 50.0)
    for _ in range(2):
        assert torch.equal(_bits(_norm(g, 50.0)), _bits(first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _norm(g, 50.0)
    side.synchronize()
    assert torch.equal(_bits(other), _bits(first))
    for scale in (2.0 ** 16, 3000.0):
        for plant in (None, INF):
            scaled = [h * scale for h in host]
            if plant is not None:
                scaled[10][CHUNK + 7] = plant                    # second chunk of the three-chunk tensor
            sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
            ga, gb = _place(scaled, layout), _place(scaled, layout)
            fa, fb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
            L.call("mc_grads_unscale_dev", _table(ga), len(ga), sc.data_ptr(), fa.data_ptr(), ops._st())
            seq = _norm(ga, 50.0)
            arr = _table(gb)
            need, ws = _workspace(arr, len(gb))
            fused = torch.full((2,), -7.0, device=DEV)
            L.call("mc_grads_unscale_norm_dev", arr, len(gb), sc.data_ptr(), fb.data_ptr(), ws.data_ptr(), need, 50.0,
                   fused.data_ptr(), ops._st())
            torch.cuda.synchronize()
            assert torch.isnan(ws[need:]).all()
            assert torch.equal(_bits(_cat(ga)), _bits(_cat(gb))), (scale, plant)
            assert torch.equal(_bits(seq), _bits(fused)), (scale, plant, seq, fused)
            assert fa.item() == fb.item() == (0.0 if plant is None else 1.0)
            assert math.isfinite(fused[0].item()) == (plant is None)
            if plant is None:
                assert abs(fused[0].double() - _norm64(gb)).item() <= EPS * _norm64(gb).item()
                if scale == 2.0 ** 16:                            # exact unscale: the norm of the unscaled originals
                    assert torch.equal(_bits(fused), _bits(first))


# ------------------------------------------------------------------------------------------------ 4. in-place clip
@pytest.mark.parametrize("layout", LAYOUTS)
def test_clip_grad_norm_in_place(layout):
    """ops.clip_grad_norm_: returns out[0] of mc_grad_norm; afterwards every gradient is BIT-equal to g_before * coef (torch's
    fp32 product with out[1]).  A max_norm above the norm leaves the gradients bit-unchanged.  The workspace it owns grows
    with the list (a 300-chunk tensor after the small set) and a single tensor is accepted like torch accepts it."""
    host = _holes(_normals(50, 3.0))
    g = _place(host, layout)
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in g]
    for p, t in zip(params, g):
        p.grad = t
    before = _cat(g).clone()
    ref = _norm(g, 25.0)
    assert 0.0 < ref[1].item() < 0.5
    got = ops.clip_grad_norm_(params, 25.0)
    assert got.dim() == 0 and got.is_cuda and torch.equal(_bits(got), _bits(ref[0]))
    assert torch.equal(_bits(_cat(g)), _bits(before * ref[1]))
    assert torch.equal(_bits(ops.grad_norm(params)), _bits(_norm(g)[0]))
    now = _cat(g).clone()
    got = ops.clip_grad_norm_(params, 1e6)
    assert torch.equal(_bits(_cat(g)), _bits(now)) and abs(got.item() - 25.0) < 1e-3
    big = torch.nn.Parameter(torch.zeros(300 * CHUNK + 5, device=DEV))
    big.grad = torch.randn(300 * CHUNK + 5, device=DEV, generator=torch.Generator(device=DEV).manual_seed(51))
    b0 = big.grad.clone()
    ref = _norm([big.grad], 100.0)
    got = ops.clip_grad_norm_(big, 100.0)
    assert torch.equal(_bits(got), _bits(ref[0])) and torch.equal(_bits(big.grad), _bits(b0 * ref[1]))
    allp = params + [big]
    ref = _norm([p.grad for p in allp], 10.0)
    got = ops.clip_grad_norm_(allp, 10.0)
    assert torch.equal(_bits(got), _bits(ref[0]))


# ------------------------------------------------------------------------------------------------ 5. clipped AdamW
KW = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)


def _flat_offsets(params):
    offs, off = [], 1
    for p in params:
        offs.append(off)
        off += (p.numel() + 3) // 4 * 4
    return offs, torch.zeros(off, device=DEV)


def _clip_ref(ref, max_norm):
    """the reference side of a clipped step: the fp64 norm through the fp32 formula, gradients multiplied in place"""
    gs = [b.grad for b in ref if b.grad is not None]
    coef = _coef_ref(_norm64(gs).float(), max_norm)
    for gr in gs:
        gr.mul_(coef)
    return coef


def test_clipped_adamw_vs_torch():
    """AdamW.step(grad_coef=) against torch.optim.AdamW(foreach=False) fed g * coef_ref, coef_ref from the fp64 norm through
    the same fp32 formula: 6 steps, gradient magnitude 10^(step % 3 - 1) (norms ~27, ~270, ~2700 against max_norm 100: the
    first of every three steps does not clip), a changing lr, gradients alternately 4 bytes off alignment.  One parameter
    has no gradient on step 0, so from step 1 on the clipped entry goes through the per-step-count launch loop.  Bounds of
    test_adamw_multi_tensor_vs_torch (rtol 2e-6; atol 2e-7 parameters, 1e-12 exp_avg_sq): the clip moves each gradient by
    at most 2 fp32 ulp.  p.grad is bit-unchanged by the fused step; the cached bf16 image of the 2-D parameter follows."""
    shapes = SIZES + [(43, 47)]
    mine = [torch.nn.Parameter(h.to(DEV)) for h in _normals(60, 1.0, shapes)]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    om, ot = AdamW(mine, **KW), torch.optim.AdamW(ref, foreach=False, **KW)
    offs, flat = _flat_offsets(mine)
    big, img0 = mine[-1], ops.cast_bf16(mine[-1])
    late, max_norm, coefs = 7, 100.0, []
    for step in range(6):
        gen = torch.Generator(device=DEV).manual_seed(160 + step)
        for i, (a, b) in enumerate(zip(mine, ref)):
            v = flat[offs[i]:offs[i] + a.numel()].view_as(a)
            v.copy_(torch.randn(a.shape, device=DEV, generator=gen) * (10.0 ** (step % 3 - 1)))
            a.grad = v if step % 2 else v.clone()
            b.grad = v.clone()
            if step == 0 and i == late:
                a.grad = b.grad = None
        for o in (om, ot):
            o.param_groups[0]["lr"] = 3e-3 * (0.5 + 0.1 * step)
        raw = [None if a.grad is None else a.grad.clone() for a in mine]
        nc = ops.grad_norm_coef(mine, max_norm)
        om.step(grad_coef=nc[1:])
        coef = _clip_ref(ref, max_norm)
        ot.step()
        coefs.append(nc[1].item())
        assert abs(nc[1].item() - coef.item()) <= 2 * EPS * coef.item(), (step, nc, coef)
        for a, r in zip(mine, raw):
            assert (a.grad is None) == (r is None) and (r is None or torch.equal(_bits(a.grad), _bits(r))), step
        img = ops.cast_bf16(big)
        assert img is img0 and torch.equal(img, big.detach().to(BF)), step
    assert [c == 1.0 for c in coefs] == [True, False, False] * 2 and min(coefs) < 0.05, coefs
    om.state_dict()
    worst = [0.0, 0.0]
    for i, (a, b) in enumerate(zip(mine, ref)):
        va, vb = om.state[a]["exp_avg_sq"], ot.state[b]["exp_avg_sq"]
        worst[0] = max(worst[0], float(((a - b).abs() - 2e-6 * b.abs()).max().detach()))
        worst[1] = max(worst[1], float(((va - vb).abs() - 2e-6 * vb.abs()).max()))
        assert float(om.state[a]["step"]) == (5.0 if i == late else 6.0)
    print(f"clipped AdamW: atol needed next to rtol 2e-6: parameters {worst[0]:.2e} (bound 2e-7), exp_avg_sq {worst[1]:.2e} (bound 1e-12)")
    for a, b in zip(mine, ref):
        torch.testing.assert_close(a, b, rtol=2e-6, atol=2e-7)
        torch.testing.assert_close(om.state[a]["exp_avg_sq"], ot.state[b]["exp_avg_sq"], rtol=2e-6, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 6. loss-scaled and clipped
def test_loss_scaled_clipped_steps_vs_torch_gradscaler():
    """LossScaler(1024, growth_interval=4).unscale_(clip=) + AdamW.step_loss_scaled(grad_coef=) against torch.amp.GradScaler:
    unscale_, the fp64-norm clip of test 5, scaler.step, update.  12 steps, an inf in one gradient on steps 1, 6 and 7.
    Skipped steps leave the parameters bit-untouched and report a non-finite norm; scale and clean-step counter are
    bit-equal to GradScaler's after every step; parameters at the tolerances of test 5."""
    shapes = SIZES + [(43, 47)]
    mine = [torch.nn.Parameter(h.to(DEV)) for h in _normals(70, 1.0, shapes)]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    om, ot = AdamW(mine, **KW), torch.optim.AdamW(ref, foreach=False, **KW)
    sm = engine.LossScaler(init_scale=1024.0, growth_interval=4)
    st = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=4)
    st.scale(torch.zeros((), device=DEV))
    bad_at = {1: 4, 6: 0, 7: 44}                                   # step -> the tensor whose gradient gets the inf
    offs, flat = _flat_offsets(mine)
    big, img0 = mine[-1], ops.cast_bf16(mine[-1])
    max_norm, clipped, scales = 100.0, 0, set()
    for step in range(12):
        scale = st.get_scale()
        scales.add(scale)
        gen = torch.Generator(device=DEV).manual_seed(270 + step)
        for i, (a, b) in enumerate(zip(mine, ref)):
            v = flat[offs[i]:offs[i] + a.numel()].view_as(a)
            v.copy_(torch.randn(a.shape, device=DEV, generator=gen) * (10.0 ** (step % 3 - 1) * scale))
            if bad_at.get(step) == i:
                v.view(-1)[v.numel() // 2] = INF
            a.grad = v if step % 2 else v.clone()
            b.grad = v.clone()
        for o in (om, ot):
            o.param_groups[0]["lr"] = 3e-3 * (0.5 + 0.1 * (step % 7))
        before = _cat([p.detach() for p in mine]).clone()
        ok, nc = sm.unscale_(mine, clip=max_norm)
        assert ok is None
        sm.update(om.step_loss_scaled(sm, grad_coef=nc[1:]))
        st.unscale_(ot)
        coef = _clip_ref(ref, max_norm)
        st.step(ot)
        st.update()
        assert sm.scale == st.get_scale() and sm.state_dict()["growth_tracker"] == int(st.state_dict()["_growth_tracker"]), step
        assert sm.last_skipped == (step in bad_at), step
        now = _cat([p.detach() for p in mine])
        if step in bad_at:
            assert torch.equal(_bits(now), _bits(before)) and not math.isfinite(nc[0].item()), step
        else:
            assert not torch.equal(now, before) and math.isfinite(nc[0].item()), step
            assert abs(nc[1].item() - coef.item()) <= 2 * EPS * coef.item(), (step, nc, coef)
            clipped += nc[1].item() < 1.0
        img = ops.cast_bf16(big)
        assert img is img0 and torch.equal(img, big.detach().to(BF)), step
        for a, b in zip(mine, ref):
            torch.testing.assert_close(a, b, rtol=2e-6, atol=2e-7, msg=lambda m_: f"step {step}: {m_}")
    assert sm.skipped == 3 and 3 <= clipped <= 6 and len(scales) >= 3, (clipped, scales)
    om.state_dict()
    for a, b in zip(mine, ref):
        torch.testing.assert_close(om.state[a]["exp_avg_sq"], ot.state[b]["exp_avg_sq"], rtol=2e-6, atol=1e-12)
        assert float(om.state[a]["step"]) == float(ot.state[b]["step"]) == 9.0


# ------------------------------------------------------------------------------------------------ 7. Trainer
@pytest.fixture(scope="module")
def b2_case():
    """weights and batches of the smallest model the GPU tests build: EfficientNet-B2 + BERT at 64 x 64, T = 16"""
    arch = oarch.build_arch("efficientnet-b2")
    sd = ow.synth_state_dict(ow.clip_shapes(arch, obert.BertShape()), seed=10)

    def batch(b):
        h = ow.synth_batch(b, 64, 64, 16, seed=3)
        return {"images": h["images"].to(DEV), "image_views": h["image_views"].to(DEV),
                "text_tokens": {k: v.to(DEV) for k, v in h["text_tokens"].items()},
                "text_tokens2": {k: v.to(DEV) for k, v in h["text_tokens2"].items()}}
    return sd, {2: batch(2), 4: batch(4)}


def _b2_trainer(sd, opt_name, **kw):
    cfg = {"name": "clip_custom", "temperature": 0.07,
           "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
           "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                            "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
           "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
    loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
    util.GlobalEnv.reset()
    model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    if opt_name == "adamw":
        opt = AdamW(list(model.parameters()), lr=5e-5, weight_decay=1e-4)
    else:
        opt = torch.optim.SGD(list(model.parameters()), lr=1e-3, momentum=0.9)
    return model, opt, engine.Trainer(model, build_loss(loss_cfg), opt, None, DEV, **kw)


@pytest.mark.parametrize("opt_name,micro,scaled", [("adamw", 1, False), ("adamw", 2, False), ("adamw", 1, True), ("sgd", 1, False)])
def test_trainer_max_grad_norm(b2_case, opt_name, micro, scaled):
    """Trainer(max_grad_norm=c) against Trainer() from identical weights, first step, c = a tenth of the plain run's norm.
    Only the clipped run's result has ``grad_norm``; it equals the fp64 norm of the unclipped gradients at rtol 4 * 2^-23
    (the 2^-23 of the kernel test plus headroom for the reference's own fp32-to-fp64 sum over ~700 tensors).  HIP AdamW:
    p.grad is left unclipped, and exp_avg of every parameter equals 0.1 * coef * grad at rtol 1e-6 (two fp32 roundings;
    atol 1e-37 keeps denormal products out of it) -- AdamW's first update itself is scale-invariant and would not show that
    the coefficient reached the kernel.  micro = 2: the micro-batched step (4 pairs, so that each micro-batch has the 2
    pairs of the single step).  scaled: a static loss scale of 1024, the fused unscale + norm.  SGD: the in-place route,
    p.grad IS clipped: its fp64 norm equals coef * grad_norm at rtol 5 * 2^-23 (one more rounding per element) and the
    momentum buffer of the first step is that clipped gradient bit for bit."""
    sd, batches = b2_case
    bt = batches[2 * micro]
    kw = dict(loss_scale=1024.0) if scaled else dict(loss_scale=None)
    model0, _, tr0 = _b2_trainer(sd, opt_name, **kw)
    out0 = tr0.step(bt, micro_batches=micro)
    assert "grad_norm" not in out0
    n0 = _norm64([p.grad for p in model0.parameters() if p.grad is not None]).item()
    assert math.isfinite(n0) and n0 > 0
    c = _f32(n0 / 10)
    model, opt, tr = _b2_trainer(sd, opt_name, max_grad_norm=c, **kw)
    out = tr.step(bt, micro_batches=micro)
    assert set(out) - set(out0) == {"grad_norm"} and out["grad_norm"].dim() == 0
    coef = tr._norm_coef[1]
    assert torch.equal(_bits(coef), _bits(_coef_ref(out["grad_norm"], c))) and abs(coef.item() - 0.1) < 1e-3
    ps = [p for p in model.parameters() if p.grad is not None]
    assert len(ps) > 100
    n1 = _norm64([p.grad for p in ps]).item()
    print(f"trainer [{opt_name} micro {micro} scaled {scaled}]: grad_norm {out['grad_norm'].item():.9g} fp64 {n1:.17g} coef {coef.item():.9g}")
    if opt_name == "adamw":
        assert abs(out["grad_norm"].item() - n1) <= 4 * EPS * n1
        for p in ps:
            torch.testing.assert_close(opt.state[p]["exp_avg"], 0.1 * coef * p.grad, rtol=1e-6, atol=1e-37)
    else:
        assert abs(out["grad_norm"].item() * coef.item() - n1) <= 5 * EPS * n1
        for p in ps:
            assert torch.equal(_bits(opt.state[p]["momentum_buffer"]), _bits(p.grad))
    # max_grad_norm = inf only reports: same result keys, coefficient exactly 1
    if opt_name == "adamw" and micro == 1 and not scaled:
        _, _, tri = _b2_trainer(sd, opt_name, max_grad_norm=INF, **kw)
        outi = tri.step(bt)
        assert "grad_norm" in outi and tri._norm_coef[1].item() == 1.0
        assert abs(outi["grad_norm"].item() - n1) <= 1e-3 * n1
