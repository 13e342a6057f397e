"""Weight EMA on the device: mc_ema_update, mc_adamw_step_ema, mc_ema_tick and what is built on them (ema.ModelEma,
AdamW.step(ema=), Trainer(ema=), save_checkpoint(ema=), Evaluator(use_ema=)).

Every comparison is on BITS.  The contract (include/mammoclip_hip.h): one applied update is s = p - e; t = w * s; e = e + t,
three separately rounded fp32 operations, w = fp32(1 - d_k) -- the three tensor operations torch performs on the CPU, which is
the reference here.

Kernel cases use the tensor set and layouts of test_grad_clip_gpu.py: sub-vector sizes, the last lane of the vector body
(1023 / 1024), a ragged tail (1027), a chunk of 16384 exactly, a second chunk of length 1, three chunks, and 35 small tensors,
so that tensor 40 onwards falls into the second launch of a call (PACK = 40 in optim.hip); zero-element tensors sit first,
across that boundary and last.  "own": one allocation each (16-byte aligned, the vector path); "flat": views that start 4
bytes past a 16-byte boundary (the scalar path) inside one nan-filled allocation whose gaps must stay nan."""
import ctypes
import types

import pytest
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import checkpoint, engine, lib as L, ops
from mammo_clip_amd.breastclip import util
from mammo_clip_amd.breastclip.evaluator import Evaluator
from mammo_clip_amd.breastclip.loss import build_loss
from mammo_clip_amd.breastclip.model import build_model
from mammo_clip_amd.breastclip.optimizer import AdamW
from mammo_clip_amd.ema import ModelEma
from oracle import arch as oarch, bert as obert, weights as ow

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = ops.BF16
CHUNK = 16384
SIZES = [1, 3, 4, 5, 1023, 1024, 1027, CHUNK, CHUNK + 1, 2 * CHUNK + 3] + [17 + i for i in range(35)]
LAYOUTS = ("own", "flat")
INF, NAN = float("inf"), float("nan")
DECAY = 0.9999
HYPER = (3e-3, 0.9, 0.999, 1e-8, 0.05)             # lr, beta1, beta2, eps, weight_decay


def _normals(seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn((s,), generator=g) * scale for s in SIZES]


def _holes(host):
    hole = torch.empty(0)
    return [hole] + host[:39] + [hole] + host[39:] + [hole]


class Placed:
    """a list of host tensors on the device in one of the two layouts; ``gaps_are_nan`` checks the bytes between flat views"""

    def __init__(self, host, layout):
        self.flat = None
        if layout == "own":
            self.t = [torch.empty_like(h, device=DEV).copy_(h) for h in host]
        else:
            offs, off = [], 1
            for h in host:
                offs.append(off)
                off += (h.numel() + 3) // 4 * 4                # the next view starts at 1 (mod 4) again
            self.flat = torch.full((off,), NAN, device=DEV)
            self.t = [self.flat[o:o + h.numel()].view(h.shape) for o, h in zip(offs, host)]
            self.gap = torch.ones(off, dtype=torch.bool, device=DEV)
            for o, h, v in zip(offs, host, self.t):
                v.copy_(h)
                self.gap[o:o + h.numel()] = False
            assert int(self.gap.sum()) > len(host)
        assert all((t.data_ptr() % 16 == 0) == (layout == "own") for t in self.t if t.numel())

    def gaps_are_nan(self):
        return self.flat is None or bool(torch.isnan(self.flat[self.gap]).all())

    def ptrs(self):
        return (ctypes.c_void_p * len(self.t))(*[t.data_ptr() if t.numel() else None for t in self.t])

    def cat(self):
        return torch.cat([t.reshape(-1) for t in self.t])


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _weight(k, decay=DECAY, warmup=True):
    """w of the k-th applied update, by the formula of the contract (double, then one rounding to fp32)"""
    d = min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay
    return torch.tensor(1.0 - d, dtype=torch.float64).float()


def _ref_update(e, p, w):
    """the contract on the CPU: three tensor operations, each rounded to fp32"""
    s = p - e
    t = s * w
    return e + t


def _numel(ts):
    return (ctypes.c_longlong * len(ts))(*[t.numel() for t in ts])


def _ema_update(sh, src, count, decay=DECAY, warmup=True, flag=None):
    L.call("mc_ema_update", sh.ptrs(), src.ptrs(), _numel(sh.t), len(sh.t), decay, int(warmup), count.data_ptr(),
           flag.data_ptr() if flag is not None else None, ops._st())


def _tick(count, flag=None):
    L.call("mc_ema_tick", count.data_ptr(), flag.data_ptr() if flag is not None else None, ops._st())


def _count(v=0):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. mc_ema_update
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("preset,warmup", [(0, True), (10 ** 6, True), (0, False)])
def test_ema_update_vs_torch_cpu(layout, preset, warmup):
    """five consecutive updates from new source values each time, against the three-operation reference: every shadow
    bit-equal after every update; the count reads preset + 5.  preset 0 with warm-up: d_k = (1 + k) / (10 + k); preset
    10^6: d_k = decay; warm-up off: decay from the first update on."""
    e_host = _holes(_normals(100))
    sh = Placed(e_host, layout)
    count = _count(preset)
    ref = torch.cat(e_host)
    for k in range(1, 6):
        p_host = _holes(_normals(100 + k, 1.0 + 0.5 * k))
        src = Placed(p_host, layout)
        _ema_update(sh, src, count, warmup=warmup)
        _tick(count)
        w = _weight(preset + k, warmup=warmup)
        ref = _ref_update(ref, torch.cat(p_host), w)
        assert _same(sh.cat(), ref), (layout, preset, k)
        assert _same(src.cat(), torch.cat(p_host)) and sh.gaps_are_nan() and src.gaps_are_nan(), k
    assert count.item() == preset + 5


# ------------------------------------------------------------------------------------------------ 2. mc_adamw_step_ema
class AdamCase:
    """parameters, gradients, both moments, shadows and (for every third tensor, in allocations of their own) bf16 images"""

    def __init__(self, layout, seed=200):
        self.p = Placed(_holes(_normals(seed)), layout)
        self.g = Placed(_holes(_normals(seed + 1, 0.1)), layout)
        self.m = Placed(_holes(_normals(seed + 2, 0.01)), layout)
        self.v = Placed(_holes([h * h for h in _normals(seed + 3, 0.1)]), layout)
        self.e = Placed(_holes(_normals(seed + 4)), layout)
        self.img = [torch.full((t.numel(),), 7.0, dtype=BF, device=DEV) if i % 3 == 0 and t.numel() else None
                    for i, t in enumerate(self.p.t)]
        self.count = _count(0)
        arr = (L.AdamwTensor * len(self.p.t))()
        for a, p, g, m, v, im in zip(arr, self.p.t, self.g.t, self.m.t, self.v.t, self.img):
            if p.numel():
                a.param, a.grad, a.exp_avg, a.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            a.numel = p.numel()
            a.bf16_image = im.data_ptr() if im is not None else None
        self.arr, self.n = arr, len(self.p.t)

    def state(self):
        return [self.p.cat(), self.m.cat(), self.v.cat(), torch.cat([i for i in self.img if i is not None]).float(),
                self.g.cat(), self.e.cat()]

    def gaps_ok(self):
        return all(x.gaps_are_nan() for x in (self.p, self.g, self.m, self.v, self.e))

    def step_ema(self, step, coef=None, flag=None, skipped=None):
        L.call("mc_adamw_step_ema", self.arr, self.e.ptrs(), self.n, *HYPER, step, DECAY, 1, self.count.data_ptr(),
               coef.data_ptr() if coef is not None else None, flag.data_ptr() if flag is not None else None,
               skipped.data_ptr() if skipped is not None else None, ops._st())

    def step_plain(self, step, coef=None, flag=None, skipped=None):
        if coef is not None:
            L.call("mc_adamw_step_clip", self.arr, self.n, *HYPER, step, coef.data_ptr(),
                   flag.data_ptr() if flag is not None else None, skipped.data_ptr() if skipped is not None else None, ops._st())
        elif flag is not None:
            L.call("mc_adamw_step_ls", self.arr, self.n, *HYPER, step, flag.data_ptr(), skipped.data_ptr(), ops._st())
        else:
            L.call("mc_adamw_step", self.arr, self.n, *HYPER, step, ops._st())


NAMES = ("parameters", "exp_avg", "exp_avg_sq", "bf16 images", "gradients", "shadows")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("clip", [False, True])
def test_adamw_step_ema_is_the_sequence(layout, clip):
    """mc_adamw_step_ema against mc_adamw_step (clip: mc_adamw_step_clip with a coefficient of 0.1) followed by mc_ema_update,
    two steps with a tick between: parameters, both moments and bf16 images bit-equal to the existing entry point, shadows
    bit-equal to the sequence, gradients untouched; the shadows also equal the CPU reference applied to the updated
    parameters."""
    a, b = AdamCase(layout), AdamCase(layout)
    coef = torch.tensor([0.1], device=DEV) if clip else None
    for step in (1, 2):
        e_before = b.e.cat().cpu()
        a.step_plain(step, coef)
        _ema_update(a.e, a.p, a.count)
        _tick(a.count)
        b.step_ema(step, coef)
        _tick(b.count)
        for name, x, y in zip(NAMES, a.state(), b.state()):
            assert _same(x, y), (layout, clip, step, name)
        assert _same(b.e.cat(), _ref_update(e_before, b.p.cat().cpu(), _weight(step))), (layout, clip, step)
        assert a.gaps_ok() and b.gaps_ok()
    assert not _same(b.e.cat(), torch.cat(_holes(_normals(204))))
    assert a.count.item() == b.count.item() == 2
    img = [i for i in b.img if i is not None]
    assert len(img) > 10 and all(_same(i, p.to(BF)) for i, p in zip(img, [p for p, i in zip(b.p.t, b.img) if i is not None]))


# ------------------------------------------------------------------------------------------------ 3. skipped steps
@pytest.mark.parametrize("layout", LAYOUTS)
def test_skipped_step_changes_nothing_and_does_not_count(layout):
    """with the non-finite flag set every array keeps its bits under the fused and the stand-alone entry and the tick leaves
    the count alone; three attempted updates with the middle one skipped equal two applied ones (k = count + 1)."""
    flag, skipped = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    clear, none_skipped = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    a, b = AdamCase(layout, 300), AdamCase(layout, 300)        # a: steps 1, 2 (skipped), 3; b: the two applied ones
    a.step_ema(1, flag=flag, skipped=skipped)
    _tick(a.count, flag)
    assert a.count.item() == 1
    flag.fill_(1.0)
    before = a.state()
    a.step_ema(2, flag=flag, skipped=skipped)
    _ema_update(a.e, a.p, a.count, flag=flag)
    _tick(a.count, flag)
    for name, x, y in zip(NAMES, before, a.state()):
        assert _same(x, y), (layout, name)
    assert a.count.item() == 1 and a.gaps_ok()
    flag.zero_()
    skipped.fill_(1.0)                                         # (what mc_loss_scale_update does for the optimizer)
    a.step_ema(3, flag=flag, skipped=skipped)
    _tick(a.count, flag)
    for step in (1, 2):
        b.step_ema(step, flag=clear, skipped=none_skipped)
        _tick(b.count, clear)
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert _same(x, y), (layout, name)
    assert a.count.item() == b.count.item() == 2
    # the stand-alone entry: update, skipped update, update == update, update
    e_host, p_host = _holes(_normals(310)), [_holes(_normals(311 + i)) for i in range(3)]
    sa, sb, ca, cb = Placed(e_host, layout), Placed(e_host, layout), _count(0), _count(0)
    for i, f in enumerate((0.0, 1.0, 0.0)):
        flag.fill_(f)
        _ema_update(sa, Placed(p_host[i], layout), ca, flag=flag)
        _tick(ca, flag)
        if f == 0.0:
            _ema_update(sb, Placed(p_host[i], layout), cb)
            _tick(cb)
        assert _same(sa.cat(), sb.cat()) and ca.item() == cb.item(), i
    assert ca.item() == 2 and sa.gaps_are_nan()
    ref = torch.cat(e_host)
    for k, i in ((1, 0), (2, 2)):
        ref = _ref_update(ref, torch.cat(p_host[i]), _weight(k))
    assert _same(sa.cat(), ref)


# ------------------------------------------------------------------------------------------------ 4. - 7. Trainer and files
CFG = {"name": "clip_custom", "temperature": 0.07,
       "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
       "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                        "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
       "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
LOSS_CFG = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
TOK = types.SimpleNamespace(vocab_size=28996)


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


def _b2_model(sd):
    util.GlobalEnv.reset()
    model = build_model(CFG, LOSS_CFG, TOK)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


def _b2_trainer(sd, opt_name, **kw):
    model = _b2_model(sd)
    if opt_name == "adamw":
        opt = AdamW(list(model.parameters()), lr=5e-5, weight_decay=1e-4)
    else:
        opt = torch.optim.SGD(list(model.parameters()), lr=1e-3, momentum=0.9)
    return model, opt, engine.Trainer(model, build_loss(LOSS_CFG), opt, None, DEV, **kw)


def _cpu_state(module):
    return {k: v.detach().to("cpu", copy=True) for k, v in module.state_dict().items()}


def _replay(shadow, live, k, decay, warmup=True):
    """one update of the contract over a whole state dict on the CPU: floats averaged with the weight of update k, integers copied"""
    w = _weight(k, decay, warmup)
    return {key: _ref_update(e, live[key], w) if e.is_floating_point() else live[key].clone() for key, e in shadow.items()}


def _assert_states_equal(got, want, what):
    assert list(got) == list(want)
    bad = [k for k in want if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or not _same(got[k], want[k])]
    assert not bad, (what, len(bad), bad[:5])


@pytest.mark.parametrize("opt_name,micro", [("adamw", 1), ("adamw", 2), ("sgd", 1)])
def test_trainer_ema_is_the_recurrence_and_changes_nothing_else(b2_case, opt_name, micro):
    """Trainer(ema=0.99) against Trainer() from identical weights, 4 deterministic steps: bit-equal losses and parameters.  The
    live state dict is copied to the CPU after every step; the three-operation recurrence replayed over those snapshots
    equals ema.module.state_dict() bit for bit after every step, num_batches_tracked equals the model's.  micro = 2: the
    micro-batched step on 4 pairs.  SGD: the stand-alone route over everything."""
    sd, batches = b2_case
    bt = batches[2 * micro]
    model0, _, tr0 = _b2_trainer(sd, opt_name, loss_scale=None, deterministic=True)
    model1, _, tr1 = _b2_trainer(sd, opt_name, loss_scale=None, deterministic=True, ema=0.99)
    ema = tr1.ema
    assert isinstance(ema, ModelEma) and tr0.ema is None and ema.decay == 0.99 and ema.warmup
    shadow = _cpu_state(model1)
    _assert_states_equal(_cpu_state(ema.module), shadow, "initial shadows")
    for k in range(1, 5):
        l0 = tr0.step(bt, micro_batches=micro)
        l1 = tr1.step(bt, micro_batches=micro)
        assert set(l0) == set(l1) and all(_same(l0[n], l1[n]) for n in l0), k
        live = _cpu_state(model1)
        shadow = _replay(shadow, live, k, 0.99)
        got = _cpu_state(ema.module)
        _assert_states_equal(got, shadow, f"shadows after step {k}")
        nbt = [key for key in live if key.endswith("num_batches_tracked")]
        assert nbt and all(got[key].dtype == torch.int64 and torch.equal(got[key], live[key]) for key in nbt)
        assert int(live[nbt[0]]) == 2 * micro * k              # two image views per pair, every micro-batch forwarded once
    assert ema.updates == 4
    _assert_states_equal(_cpu_state(model1), _cpu_state(model0), "live weights with and without EMA")
    assert not ema.module.training and not any(p.requires_grad for p in ema.module.parameters())
    moved = [key for key, v in shadow.items() if v.is_floating_point() and not _same(v, sd[key])]
    assert len(moved) > len(shadow) // 2, len(moved)


def test_trainer_ema_under_a_loss_scaler_skips_with_the_step(b2_case):
    """an explicit LossScaler; step 1 has an inf written into one gradient before the optimizer step: shadows (integer ones
    included) and ``updates`` are unchanged by it and skipped_steps is 1; the following clean step averages with k = 1."""
    sd, batches = b2_case
    model, _, tr = _b2_trainer(sd, "adamw", loss_scale=engine.LossScaler(init_scale=16.0), deterministic=True, ema=0.99)
    ema = tr.ema
    first = _cpu_state(ema.module)
    inner = tr._optimizer_step

    def poisoned():
        g = next(p.grad for p in model.parameters() if p.grad is not None and p.numel() > 8)
        g.view(-1)[3] = INF
        inner()
    tr._optimizer_step = poisoned
    out = tr.step(batches[2])
    assert out["skipped_steps"].item() == 1 and tr.scaler.last_skipped
    assert ema.updates == 0
    _assert_states_equal(_cpu_state(ema.module), first, "shadows after a skipped step")
    nbt = "image_encoder._bn0.num_batches_tracked"
    assert int(first[nbt]) == 0 and int(model.state_dict()[nbt]) == 2      # the forward ran; the shadow counter did not follow
    _assert_states_equal({k: v for k, v in _cpu_state(model).items() if v.is_floating_point() and "running_" not in k},
                         {k: v for k, v in sd.items() if v.is_floating_point() and "running_" not in k}, "weights after a skipped step")
    tr._optimizer_step = inner
    out = tr.step(batches[2])
    assert out["skipped_steps"].item() == 1 and not tr.scaler.last_skipped
    assert ema.updates == 1
    live = _cpu_state(model)
    _assert_states_equal(_cpu_state(ema.module), _replay(first, live, 1, 0.99), "shadows after the first applied step")
    assert int(live["image_encoder._bn0.num_batches_tracked"]) == 4       # both steps were forwarded (two image views each)


def _embed(model, batch):
    ev = Evaluator(model=model, device=DEV)
    return ev.encode_image(batch["images"], as_tensor=True).clone(), ev.encode_text(batch["text_tokens"], as_tensor=True).clone()


def test_averaged_module_never_reads_stale_weight_images(b2_case):
    """embeddings of ema.module through the Evaluator (which caches bf16 weight images of it), one training step, embeddings
    again: bit-equal to those of a freshly built model loaded from ema.state_dict()["module"], and not those from before."""
    sd, batches = b2_case
    bt = batches[2]
    model, _, tr = _b2_trainer(sd, "adamw", loss_scale=None, ema=0.9)
    img0, txt0 = _embed(tr.ema.module, bt)
    assert _same(img0, _embed(model, bt)[0])
    tr.step(bt)
    img1, txt1 = _embed(tr.ema.module, bt)
    fresh = _b2_model(tr.ema.state_dict()["module"])
    imgf, txtf = _embed(fresh, bt)
    assert _same(img1, imgf) and _same(txt1, txtf)
    assert not _same(img1, img0) and not _same(txt1, txt0)
    assert tr.ema.updates == 1


def test_checkpoint_round_trip_and_evaluator(b2_case, tmp_path):
    """save_checkpoint(ema=) then load_checkpoint into a new ModelEma: shadows bit for bit, updates, decay and warm-up; one
    further update from identical model weights gives identical shadows in both; Evaluator(ckpt_path, use_ema=True) gives
    ema.module's embeddings and raises KeyError on a checkpoint saved without EMA.  The trainer is handed a ModelEma that was
    built from another instance of the model (identical weights) and binds it to its own."""
    sd, batches = b2_case
    bt = batches[2]
    model, opt, tr = _b2_trainer(sd, "adamw", loss_scale=None, ema=ModelEma(_b2_model(sd), decay=0.97, warmup=False))
    ema = tr.ema
    for _ in range(2):
        tr.step(bt)
    cfg = {"model": CFG, "loss": LOSS_CFG}
    path = checkpoint.save_checkpoint(str(tmp_path / "ema.tar"), model, config=cfg, ema=ema)
    model2 = _b2_model(sd)
    ema2 = ModelEma(model2, decay=0.5, warmup=True)
    ckpt = checkpoint.load_checkpoint(path, model2, ema=ema2)
    assert ckpt["ema"] == {"decay": 0.97, "warmup": False, "updates": 2}
    assert (ema2.decay, ema2.warmup, ema2.updates) == (0.97, False, 2)
    want = _cpu_state(ema.module)
    _assert_states_equal(_cpu_state(ema2.module), want, "restored shadows")
    _assert_states_equal(_cpu_state(model2), _cpu_state(model), "restored weights")
    assert not _same(want["logit_scale"], _cpu_state(model)["logit_scale"])
    emb = _embed(ema.module, bt)
    ev = Evaluator(ckpt_path=path, tokenizer=TOK, device=DEV, use_ema=True)
    assert _same(ev.encode_image(bt["images"], as_tensor=True), emb[0])
    assert _same(ev.encode_text(bt["text_tokens"], as_tensor=True), emb[1])
    assert not _same(_embed(model, bt)[0], emb[0])
    ema.update(model)
    ema2.update(model2)
    assert ema.updates == ema2.updates == 3
    after = _cpu_state(ema2.module)
    _assert_states_equal(after, _cpu_state(ema.module), "shadows one update after the restore")
    _assert_states_equal(after, _replay(want, _cpu_state(model), 3, 0.97, warmup=False), "that update against the contract")
    plain = checkpoint.save_checkpoint(str(tmp_path / "plain.tar"), model, config=cfg)
    with pytest.raises(KeyError):
        Evaluator(ckpt_path=plain, tokenizer=TOK, device=DEV, use_ema=True)
