"""SGD with momentum on the device: mc_sgd_step and what is built on it (breastclip.optimizer.SGD, build_optimizer, the Trainer's
fused routes).  Every comparison with tests/_sgd_ref.py -- the rule of include/mammoclip_hip.h with one torch CPU operation per
rounding -- is on BITS; only the comparisons with torch.optim.SGD itself (which fuses alpha * x + y) use the bound test_sgd.py
derives: |x - y| <= k * 2^-24 * A * 1.01, k = 6 for the buffer and 10 for the parameter, A computed on the CPU in float64.

Kernel cases: every tensor of a call is a view of ONE nan-filled allocation per array, "own" at 16-byte aligned offsets (the
vector bodies and the ragged tail), "off1" one element past them (the scalar body; the image 2 bytes past 8-byte alignment).
Whole allocations are compared, so the bytes between the views must keep their nan (the image's filler its 7.0).  Momentum
buffers start as nan: a first step that read its buffer would show.  Every other tensor has a 16-bit image."""
import copy
import ctypes
import types

import pytest
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import engine, lib as L, ops
from mammo_clip_amd.breastclip import util
from mammo_clip_amd.breastclip.loss import build_loss
from mammo_clip_amd.breastclip.model import build_model
from mammo_clip_amd.breastclip.optimizer import SGD, build_optimizer
from mammo_clip_amd.ema import ModelEma
from oracle import arch as oarch, bert as obert, weights as ow

import _sgd_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = ops.BF16
CHUNK = 16384
SIZES = [1, 3, 4, 5, 1023, 1024, 1027, 2047, 2048, 2051, 3075, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1027]
LAYOUTS = ("own", "off1")
NAN, INF = float("nan"), float("inf")
LR, DECAY = 0.05, 0.9
COMBOS = R.combos()


def _id(c):
    return "mu{momentum}-damp{dampening}-nest{nesterov:d}-wd{weight_decay}-max{maximize:d}".format(**c)


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Flat:
    """where the tensors of a call lie inside one allocation"""

    def __init__(self, sizes, layout):
        self.sizes, self.offs = list(sizes), []
        off = 0 if layout == "own" else 1
        for s in sizes:
            self.offs.append(off)
            off += (s + 3) // 4 * 4 + (4 if s == 0 else 0)
        self.total = off + 4
        self.mask = torch.zeros(self.total, dtype=torch.bool)
        for o, s in zip(self.offs, sizes):
            self.mask[o:o + s] = True

    def host(self, values, fill=NAN, dtype=torch.float32):
        """values: one flat tensor of sum(sizes) elements -> the allocation's content"""
        flat = torch.full((self.total,), fill, dtype=dtype)
        flat[self.mask] = values.to(dtype)
        return flat

    def ptr(self, dev, i):
        return dev.data_ptr() + self.offs[i] * dev.element_size() if self.sizes[i] else None


def _randn(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


class Case:
    """one call's arrays on the device and the reference state on the host (flat tensors of sum(sizes) elements)"""

    def __init__(self, sizes, layout, momentum, seed=1, images=True):
        self.lay, self.n, self.mom = Flat(sizes, layout), sum(sizes), momentum != 0
        lay = self.lay
        self.p_ref, self.e_ref, self.b_ref = _randn(self.n, seed), _randn(self.n, seed + 1), None
        self.p, self.e = lay.host(self.p_ref).to(DEV), lay.host(self.e_ref).to(DEV)
        self.g = torch.full((lay.total,), NAN, device=DEV)
        self.b = torch.full((lay.total,), NAN, device=DEV) if self.mom else None
        self.has_img = [images and i % 2 == 0 and s > 0 for i, s in enumerate(sizes)]
        self.img_mask = torch.zeros(lay.total, dtype=torch.bool)
        for o, s, h in zip(lay.offs, sizes, self.has_img):
            self.img_mask[o:o + s] = h
        self.img = torch.full((lay.total,), 7.0, dtype=BF, device=DEV)
        self.img_ref = torch.full((lay.total,), 7.0, dtype=BF)     # (an image is written by an APPLIED step only)
        self.count = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.updates = 0
        arr = (L.AdamwTensor * len(sizes))()
        for i, (a, s) in enumerate(zip(arr, sizes)):
            a.param, a.grad, a.numel = lay.ptr(self.p, i), lay.ptr(self.g, i), s
            a.exp_avg = lay.ptr(self.b, i) if self.mom else None
            a.bf16_image = lay.ptr(self.img, i) if self.has_img[i] else None
        self.arr = arr
        self.shadows = (ctypes.c_void_p * len(sizes))(*[lay.ptr(self.e, i) for i in range(len(sizes))])
        vec = [lay.ptr(self.p, i) % 16 == 0 for i, s in enumerate(sizes) if s]
        assert all(vec) if layout == "own" else not any(vec)

    def set_grad(self, g):
        self.g_host = g
        self.g.copy_(self.lay.host(g))

    def launch(self, step, hyper, coef=None, ema=False, flag=None, skipped=None):
        L.call("mc_sgd_step", self.arr, self.shadows if ema else None, len(self.lay.sizes), LR, hyper["momentum"], hyper["dampening"],
               hyper["weight_decay"], int(hyper["nesterov"]), int(hyper["maximize"]), step, DECAY, 1, self.count.data_ptr(),
               coef.data_ptr() if coef is not None else None, flag.data_ptr() if flag is not None else None,
               skipped.data_ptr() if skipped is not None else None, ops._st())

    def tick(self, flag=None):
        L.call("mc_ema_tick", self.count.data_ptr(), flag.data_ptr() if flag is not None else None, ops._st())

    def ref_step(self, hyper, coef=None, ema=False):
        """one applied step of the restatement on the whole flat state"""
        self.p_ref, self.b_ref = R.sgd_step(self.p_ref, self.g_host, self.b_ref, lr=LR, coef=coef.cpu() if coef is not None else None, **hyper)
        self.img_ref[self.img_mask] = self.lay.host(self.p_ref).to(BF)[self.img_mask]
        if ema:
            self.updates += 1
            self.e_ref = R.ema_update(self.e_ref, self.p_ref, R.ema_weight(self.updates, DECAY))

    def check(self, what):
        lay = self.lay
        assert _same(self.p, lay.host(self.p_ref)), (what, "parameters")
        assert _same(self.g, lay.host(self.g_host)), (what, "gradients")
        assert _same(self.e, lay.host(self.e_ref)), (what, "shadows")
        if self.mom:
            want = lay.host(self.b_ref) if self.b_ref is not None else torch.full((lay.total,), NAN)
            assert _same(self.b, want), (what, "momentum buffers")
        assert _same(self.img, self.img_ref), (what, "16-bit images")


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("combo", COMBOS, ids=_id)
def test_kernel_vs_restatement(layout, combo):
    """every size, three steps (first step, recurrence twice) with new gradients each, without a clip coefficient and with 0.1 and
    1.0, without and with EMA shadows (decay 0.9 with warm-up, the count ticked between steps): parameters, buffers, shadows,
    images, the untouched gradients and every byte between them after every step"""
    for ci, cv in enumerate((None, 0.1, 1.0)):
        coef = torch.tensor([cv], device=DEV) if cv is not None else None
        for ema in (False, True):
            c = Case(SIZES, layout, combo["momentum"], seed=10 * ci + ema)
            for step in (1, 2, 3):
                c.set_grad(_randn(c.n, 100 + step, 0.5 * step))
                c.launch(step, combo, coef, ema)
                if ema:
                    c.tick()
                c.ref_step(combo, coef, ema)
                c.check((layout, cv, ema, step))
            assert c.count.item() == (3 if ema else 0)
            assert not _same(c.p, c.lay.host(_randn(c.n, 10 * ci + ema)))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_tensors", [41, 81])
def test_kernel_across_launch_packs(layout, n_tensors):
    """41 and 81 small tensors in one call (40 per launch), empty ones first, at the pack boundary and last, with everything on:
    nesterov momentum, weight decay, a clip coefficient, EMA, images; and plain SGD (no buffer pointer at all)"""
    sizes = [17 + i for i in range(n_tensors)]
    sizes = [0] + sizes[:39] + [0] + sizes[39:] + [0]
    coef = torch.tensor([0.1], device=DEV)
    for hyper, ema in ((dict(momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-2, maximize=False), True),
                       (dict(momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0, maximize=False), False)):
        c = Case(sizes, layout, hyper["momentum"], seed=5)
        for step in (1, 2, 3):
            c.set_grad(_randn(c.n, 200 + step))
            c.launch(step, hyper, coef, ema)
            c.tick()
            c.ref_step(hyper, coef, ema)
            c.check((layout, n_tensors, step))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bad_step", [1, 2])
def test_kernel_loss_scale_skips(layout, bad_step):
    """three attempted steps, the flag set on one of them: that launch changes nothing by a bit (buffers keep their nan when it
    was step 1, and the NEXT step is then the first one: buf = g'), the EMA count stays; the host passes the attempted step
    count and the device counter of skipped steps, as the optimizer does"""
    hyper = dict(momentum=0.9, dampening=0.5, nesterov=False, weight_decay=1e-2, maximize=False)
    flag, skipped = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    coef = torch.tensor([0.1], device=DEV)
    c = Case(SIZES, layout, 0.9, seed=7)
    for step in (1, 2, 3):
        bad = step == bad_step
        flag.fill_(1.0 if bad else 0.0)
        c.set_grad(_randn(c.n, 300 + step))
        c.launch(step, hyper, coef, True, flag, skipped)
        c.tick(flag)
        if bad:
            skipped += 1.0                                       # (what mc_loss_scale_update does for the optimizer)
        else:
            c.ref_step(hyper, coef, True)
        c.check((layout, bad_step, step))
        assert c.count.item() == c.updates == step - (step >= bad_step)
    if bad_step == 1:
        assert c.b_ref is not None and c.updates == 2


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_pass_is_the_sequence(layout):
    """the pass with clip + EMA against one call per stage: mc_grads_scale_dev on the gradients, the plain pass, mc_ema_update,
    mc_ema_tick -- two steps, parameters, buffers, shadows and images bit-equal"""
    hyper = dict(momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-2, maximize=True)
    coef = torch.tensor([0.1], device=DEV)
    a, b = Case(SIZES, layout, 0.9, seed=9), Case(SIZES, layout, 0.9, seed=9)
    n = len(SIZES)
    for step in (1, 2):
        g = _randn(a.n, 400 + step)
        a.set_grad(g)
        b.set_grad(g)
        L.call("mc_grads_scale_dev", a.arr, n, coef.data_ptr(), ops._st())
        a.launch(step, hyper)
        src = (ctypes.c_void_p * n)(*[a.lay.ptr(a.p, i) for i in range(n)])
        L.call("mc_ema_update", a.shadows, src, (ctypes.c_longlong * n)(*SIZES), n, DECAY, 1, a.count.data_ptr(), None, ops._st())
        a.tick()
        b.launch(step, hyper, coef, True)
        b.tick()
        for name in ("p", "b", "e", "img"):
            assert _same(getattr(a, name), getattr(b, name)), (layout, step, name)
        assert _same(b.g, b.lay.host(g)) and not _same(a.g, b.g)
    assert a.count.item() == b.count.item() == 2


# ------------------------------------------------------------------------------------------------ 2. the class
SHAPES = [(43, 47), (1027,), (CHUNK + 1,), (5,), (64, 64)]


def _param_set(seed=20):
    return [torch.nn.Parameter((_randn(int(torch.Size(s).numel()), seed + i)).view(s).to(DEV)) for i, s in enumerate(SHAPES)]


def _within(x, y, k, a, what):
    err = (x.detach().cpu().double() - y.detach().cpu().double()).abs().reshape(-1)
    lim = k * R.U * a.reshape(-1) * 1.01
    assert bool((err <= lim).all()), (what, float((err / (R.U * a.reshape(-1))).max()))
    return float((err / (R.U * a.reshape(-1)).clamp_min(1e-300)).max())


def _torch_twin(mine, kw):
    ref = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    return ref, torch.optim.SGD(ref, lr=LR, foreach=False, **kw)


@pytest.mark.parametrize("combo", COMBOS, ids=_id)
def test_class_vs_torch_sgd_on_the_device(combo):
    """SGD against torch.optim.SGD on the same device, ONE step at a time from a copied state: a first step, then -- torch's
    parameters and buffers overwritten with this class's, so both start from identical state again -- a later one.  Within the
    derived bound; the class itself is also bit-equal to the restatement."""
    mine = _param_set()
    om = SGD(mine, lr=LR, **combo)
    ref, ot = _torch_twin(mine, combo)
    worst = [0.0, 0.0]
    for step in (1, 2):
        p0 = [p.detach().cpu().clone() for p in mine]
        b0 = [om.state[p]["momentum_buffer"].cpu().clone() if step > 1 and combo["momentum"] else None for p in mine]
        for i, (a, b) in enumerate(zip(mine, ref)):
            a.grad = _randn(a.numel(), 500 + 10 * step + i, 0.3).view_as(a).to(DEV)
            b.grad = a.grad.clone()
        om.step()
        ot.step()
        for i, (a, b) in enumerate(zip(mine, ref)):
            g = a.grad.cpu()
            p32, b32 = R.sgd_step(p0[i], g, b0[i], lr=LR, **combo)
            assert _same(a, p32), (step, i)
            _p64, _b64, a_p, a_b = R.fp64_step(p0[i], g, b0[i], lr=LR, **combo)
            worst[0] = max(worst[0], _within(a, b, R.K_P, a_p, ("parameter", step, i)))
            if combo["momentum"]:
                assert _same(om.state[a]["momentum_buffer"], b32), (step, i)
                worst[1] = max(worst[1], _within(om.state[a]["momentum_buffer"], ot.state[b]["momentum_buffer"], R.K_BUF, a_b, ("buffer", step, i)))
            else:
                assert a not in om.state and len(ot.state[b]) == 0
        with torch.no_grad():
            for a, b in zip(mine, ref):
                b.copy_(a)
                if combo["momentum"]:
                    ot.state[b]["momentum_buffer"].copy_(om.state[a]["momentum_buffer"])
    print(f"{_id(combo)}: |SGD - torch.optim.SGD| in units of 2^-24 A: p {worst[0]:.2f} (bound 10), buf {worst[1]:.2f} (bound 6)")


def test_class_images_groups_and_late_parameters():
    """two groups (momentum 0.9 with nesterov; plain), a cached 16-bit image of one parameter, a clip coefficient: three steps
    against the restatement.  The last parameter of group 0 gets its first gradient on step 3 and takes buf = g' then, the others
    go on with their recurrence; before that it has no state.  A non-contiguous gradient is accepted; the image stays the same
    object, current and equal to the cast after every step."""
    ps = _param_set(30)
    kw0 = dict(momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-2, maximize=False)
    kw1 = dict(momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0, maximize=False)
    opt = SGD([dict(params=ps[:3], **kw0), dict(params=ps[3:], **kw1)], lr=LR)
    r0, r1 = R.Replay(ps[:3], lr=LR, **kw0), R.Replay(ps[3:], lr=LR, **kw1)
    img0 = ops.cast_bf16(ps[0])
    coef = torch.tensor([0.5], device=DEV)
    for step in (1, 2, 3):
        for i, p in enumerate(ps):
            p.grad = _randn(p.numel(), 600 + 10 * step + i).view_as(p).to(DEV)
        ps[4].grad = ps[4].grad.t().contiguous().t()             # same values, column-major
        assert not ps[4].grad.is_contiguous()
        if step < 3:
            ps[2].grad = None
        opt.step(grad_coef=coef)
        r0.step([p.grad for p in ps[:3]], coef=coef)
        r1.step([p.grad for p in ps[3:]], coef=coef)
        for i, p in enumerate(ps):
            want = (r0.p + r1.p)[i]
            assert _same(p, want.view_as(p)), (step, i)
        sd = opt.state_dict()["state"]
        assert set(sd) == ({0, 1} if step < 3 else {0, 1, 2})
        for i in sd:
            assert set(sd[i]) == {"momentum_buffer"} and _same(sd[i]["momentum_buffer"], r0.buf[i].view_as(ps[i])), (step, i)
        img = ops.cast_bf16(ps[0])
        assert img is img0 and torch.equal(img, ps[0].detach().to(BF)), step


class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(37, 29)
        self.b = torch.nn.Linear(29, 700)


@pytest.mark.parametrize("bad", [(1,), (2,), (1, 2)])
def test_class_loss_scaled_steps(bad):
    """LossScaler.unscale_ + SGD.step_loss_scaled(ema=) + ModelEma.update + LossScaler.update, three steps with an inf in one
    gradient on the steps of ``bad``: a skipped step changes no parameter, buffer or shadow by a bit; the step after a skipped
    first step is a first step; the optimizer's counter of skipped steps and the EMA count move only with what happened;
    state_dict() has no momentum_buffer while every step so far was skipped, and every buffer afterwards."""
    torch.manual_seed(3)
    model = TinyNet().to(DEV)
    ps = list(model.parameters())
    kw = dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=1e-2, maximize=False)
    opt = SGD(ps, lr=LR, **kw)
    ema = ModelEma(model, decay=DECAY)
    scaler = engine.LossScaler(init_scale=4.0)
    rep = R.Replay(ps, shadows=ps, decay=DECAY, lr=LR, **kw)
    applied = 0
    for step in (1, 2, 3):
        scale = scaler.scale
        for i, p in enumerate(ps):
            p.grad = (_randn(p.numel(), 700 + 10 * step + i) * scale).view_as(p).to(DEV)
        if step in bad:
            ps[1].grad.view(-1)[3] = INF
        before = [p.detach().clone() for p in ps]
        assert scaler.unscale_(ps) is None
        grads = [p.grad.clone() for p in ps]
        flag = scaler.state(DEV)[scaler._FLAG:scaler._FLAG + 1]
        counter = opt.step_loss_scaled(scaler, ema=ema)
        ema.update(model, found_inf=flag)
        scaler.update(counter)
        rep.step(grads, skipped=step in bad)
        applied += step not in bad
        assert scaler.last_skipped == (step in bad)
        assert counter.item() == step - applied and ema.updates == applied == rep.updates
        if step in bad:
            assert all(_same(p, q) for p, q in zip(ps, before)), step
        for i, p in enumerate(ps):
            assert _same(p, rep.p[i].view_as(p)), (step, i)
            assert _same(ema.shadows_for([p])[0], rep.e[i].view_as(p)), (step, i)
        sd = opt.state_dict()["state"]
        if applied == 0:
            assert sd == {} and not any("momentum_buffer" in opt.state.get(p, {}) for p in ps)
        else:
            assert set(sd) == set(range(len(ps)))
            assert all(_same(sd[i]["momentum_buffer"], rep.buf[i].view_as(ps[i])) for i in sd), step
    assert scaler.skipped == len(bad)


@pytest.mark.parametrize("direction", ["hip_to_torch", "torch_to_hip"])
def test_checkpoint_round_trip_with_torch_sgd(direction):
    """two steps under one class, state_dict() loaded into the other, one further step under both from identical parameters:
    the loaded momentum buffers are the saved ones bit for bit, and buffers and parameters after the step agree within the
    single-step bound"""
    kw = dict(momentum=0.9, dampening=0.5, nesterov=False, weight_decay=1e-2, maximize=False)
    src_p = _param_set(40)
    dst_p = [torch.nn.Parameter(p.detach().clone()) for p in src_p]
    make_hip, make_torch = (lambda ps: SGD(ps, lr=LR, **kw)), (lambda ps: torch.optim.SGD(ps, lr=LR, foreach=False, **kw))
    src, dst = (make_hip(src_p), make_torch(dst_p)) if direction == "hip_to_torch" else (make_torch(src_p), make_hip(dst_p))
    for step in (1, 2):
        for i, p in enumerate(src_p):
            p.grad = _randn(p.numel(), 800 + 10 * step + i, 0.3).view_as(p).to(DEV)
        src.step()
    sd = copy.deepcopy(src.state_dict())
    assert set(sd["state"]) == set(range(len(src_p))) and all(set(v) == {"momentum_buffer"} for v in sd["state"].values())
    dst.load_state_dict(sd)
    with torch.no_grad():
        for a, b in zip(src_p, dst_p):
            b.copy_(a)
    assert all(_same(dst.state[b]["momentum_buffer"], src.state[a]["momentum_buffer"]) for a, b in zip(src_p, dst_p))
    p0 = [p.detach().cpu().clone() for p in src_p]
    b0 = [src.state[p]["momentum_buffer"].cpu().clone() for p in src_p]
    for i, (a, b) in enumerate(zip(src_p, dst_p)):
        a.grad = _randn(a.numel(), 850 + i, 0.3).view_as(a).to(DEV)
        b.grad = a.grad.clone()
    src.step()
    dst.step()
    dst.state_dict()
    for i, (a, b) in enumerate(zip(src_p, dst_p)):
        _p64, _b64, a_p, a_b = R.fp64_step(p0[i], a.grad.cpu(), b0[i], lr=LR, **kw)
        _within(a, b, R.K_P, a_p, (direction, "parameter", i))
        _within(src.state[a]["momentum_buffer"], dst.state[b]["momentum_buffer"], R.K_BUF, a_b, (direction, "buffer", i))
        hip = a if direction == "hip_to_torch" else b
        p32, b32 = R.sgd_step(p0[i], a.grad.cpu(), b0[i], lr=LR, **kw)
        assert _same(hip, p32) and _same((src if direction == "hip_to_torch" else dst).state[hip]["momentum_buffer"], b32), i


# ------------------------------------------------------------------------------------------------ 3. the Trainer
CFG = {"name": "clip_custom", "temperature": 0.07,
       "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
       "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                        "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
       "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
LOSS_CFG = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
SGD_CFG = {"lr": 1e-3, "momentum": 0.9, "weight_decay": 1e-4, "nesterov": True}


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


TRAINER_CASES = {
    "single": (1, {}),
    "micro2": (2, {}),
    "static-loss-scale": (1, dict(loss_scale=1024.0)),
    "clipped": (1, dict(max_grad_norm=1e-3)),
    "ema": (1, dict(ema=0.99)),
    "all-frozen-bn-deterministic": (2, dict(loss_scale=1024.0, max_grad_norm=1e-3, ema=0.99, deterministic=True)),
}


@pytest.mark.parametrize("case", list(TRAINER_CASES))
def test_trainer_steps_are_the_replay(b2_case, case, monkeypatch):
    """build_optimizer("sgd") under the Trainer, two steps on the small model (4 pairs when micro-batched): the parameters after
    each step are the restatement applied on the CPU to the parameters before it and the gradients the step left in ``p.grad``
    (unscaled in place under a loss scale; NOT clipped: the coefficient reaches the kernel), bit for bit; with ``ema`` the
    shadows of the parameters too.  The 16-bit weight images the forward cached are the same objects after every step, current
    (stamped with the parameter's version: the next forward hits the cache) and equal to the cast of the updated parameter.  No step reads the device on the host: the
    flag read of the slow branch (``unscale_(sync=True)``) and the in-place clip must not be called."""
    micro, kw = TRAINER_CASES[case]
    sd, batches = b2_case
    util.GlobalEnv.reset()
    model = build_model(CFG, LOSS_CFG, types.SimpleNamespace(vocab_size=28996))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    if "frozen" in case:
        model.image_encoder.freeze_bn()
    opt = build_optimizer(model, {"name": "sgd", "config": SGD_CFG})
    assert type(opt) is SGD
    tr = engine.Trainer(model, build_loss(LOSS_CFG), opt, None, DEV, **dict(dict(loss_scale=None), **kw))
    ps = [p for p in model.parameters()]
    unscale = engine.LossScaler.unscale_

    def no_sync(self, params, sync=False, clip=None):
        assert not sync, "the HIP SGD takes the route without a flag read"
        return unscale(self, params, sync=sync, clip=clip)
    monkeypatch.setattr(engine.LossScaler, "unscale_", no_sync)
    monkeypatch.setattr(ops, "grads_scale_", lambda *a, **k: pytest.fail("the HIP SGD clips inside its pass"))
    rep, images = None, None
    for step in (1, 2):
        if rep is None:                                          # (afterwards the replay's own state is the state before)
            before = [p.detach().cpu() for p in ps]
            rep = R.Replay(before, shadows=before if tr.ema is not None else None, decay=0.99,
                           **dict(SGD_CFG, dampening=0.0, maximize=False))
        out = tr.step(batches[2 * micro], micro_batches=micro)
        assert torch.isfinite(out["total"]).all()
        live = [i for i, p in enumerate(ps) if p.grad is not None]
        assert len(live) > 100
        coef = tr._norm_coef[1:].cpu() if "max_grad_norm" in kw else None
        if coef is not None:
            assert 0.0 < coef.item() < 1.0, "the case is meant to clip"
        rep.step([p.grad for p in ps], coef=coef)
        bad = [i for i, p in enumerate(ps) if not _same(p, rep.p[i].view_as(p))]
        assert not bad, (case, step, len(bad), bad[:5])
        if tr.ema is not None:
            bad = [i for i in live if not _same(tr.ema.shadows_for([ps[i]])[0], rep.e[i].view_as(ps[i]))]
            assert not bad and tr.ema.updates == step, (case, step, len(bad))
        if tr.scaler is not None:
            assert out["skipped_steps"].item() == 0
        found = ops.cached_cast_images([ps[i] for i in live])
        if images is None:
            images = {k: v[1] for k, v in found.items()}
            assert len(images) > 50
        assert set(found) == set(images) and all(found[k][1] is images[k] for k in images), (case, step)
        for p in ps:
            if id(p) in images:                                  # (the forward caches images of 2-D views: look up by the cache's key)
                _ref, version, val = ops._WCACHE[found[id(p)][0]]
                assert val is images[id(p)] and version == p._version, (case, step)
                assert torch.equal(val.reshape(-1), p.detach().to(BF).reshape(-1)), (case, step)
    sdo = opt.state_dict()["state"]
    assert len(sdo) == len(live) and all(set(v) == {"momentum_buffer"} for v in sdo.values())
