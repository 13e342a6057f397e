"""Weight EMA, host side (no HIP kernel is launched here): the decay schedule and its fp32 weight, argument checks of
``ema.ModelEma`` and of the three entry points, the layout of the averaged module and of the checkpoint keys, and the
refusal to update CPU tensors.  The arithmetic itself is tested on the device in test_ema_gpu.py."""
import ctypes
import struct
import types

import pytest
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import checkpoint, lib as L
from mammo_clip_amd.breastclip import util
from mammo_clip_amd.breastclip.model import build_model
from mammo_clip_amd.ema import ModelEma

CFG = {"name": "clip_custom", "temperature": 0.07,
       "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
       "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                        "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
       "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}


@pytest.fixture(scope="module")
def model():
    util.GlobalEnv.reset()
    return build_model(CFG, {"breast_clip": {}}, types.SimpleNamespace(vocab_size=28996))


def _tiny():
    m = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    return m


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


@pytest.mark.parametrize("warmup", [True, False])
def test_decay_at_is_the_formula(warmup):
    """d_k = min(decay, (1 + k) / (10 + k)) in double with warm-up, decay without; w = fp32(1 - d_k)"""
    ema = ModelEma(_tiny(), decay=0.9999, warmup=warmup)
    for k in (1, 2, 9, 10 ** 6):
        want = min(0.9999, (1.0 + k) / (10.0 + k)) if warmup else 0.9999
        assert ema.decay_at(k) == want, k
        assert ema.weight_at(k) == _f32(1.0 - want), k
        assert ema.weight_at(k) == float(torch.tensor(1.0 - want, dtype=torch.float64).float()), k
    if warmup:
        assert ema.decay_at(1) == 2.0 / 11.0 and ema.decay_at(2) == 0.25 and ema.decay_at(9) == 10.0 / 19.0
    assert ema.decay_at(10 ** 6) == 0.9999                      # (1e6 + 1) / (1e6 + 10) = 0.999991 > decay
    assert ModelEma(_tiny(), decay=0.5).decay_at(9) == 0.5       # the decay caps the warm-up from below 10 / 19 on
    with pytest.raises(ValueError):
        ema.decay_at(0)


def test_constructor_argument_checks():
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ModelEma(_tiny(), decay=bad)
    with pytest.raises(TypeError):
        ModelEma([torch.zeros(3)], decay=0.9)
    ema = ModelEma(_tiny())
    assert ema.decay == 0.9999 and ema.warmup is True and ema.updates == 0
    with pytest.raises(ValueError):
        ema.load_state_dict(dict(ema.state_dict(), decay=1.0))


def test_module_has_the_models_layout(model):
    """ema.module.state_dict(): the model's keys in the model's order, fp32 floats and int64 counters, equal values in storages
    of its own; eval mode, nothing requires a gradient, and the model itself is left as it was"""
    model.train()
    ema = ModelEma(model, decay=0.99)
    sd, esd = model.state_dict(), ema.module.state_dict()
    assert list(esd.keys()) == list(sd.keys()) and len(esd) == 710
    n_int = 0
    for k in sd:
        assert esd[k].dtype == (torch.float32 if sd[k].is_floating_point() else torch.int64), k
        assert esd[k].shape == sd[k].shape and torch.equal(esd[k], sd[k]), k
        assert esd[k].data_ptr() != sd[k].data_ptr() or sd[k].numel() == 0, k
        n_int += not sd[k].is_floating_point()
    assert n_int > 0 and any(k.endswith("num_batches_tracked") for k in sd)
    assert not ema.module.training and model.training
    assert not any(p.requires_grad for p in ema.module.parameters()) and any(p.requires_grad for p in model.parameters())
    st = ema.state_dict()
    assert set(st) == {"module", "decay", "warmup", "updates"} and list(st["module"].keys()) == list(sd.keys())
    assert (st["decay"], st["warmup"], st["updates"]) == (0.99, True, 0)
    assert all(v.device.type == "cpu" for v in st["module"].values())


def test_checkpoint_key_layout(model, tmp_path):
    """"model" is untouched by passing ema=; "model_ema" has its layout, "ema" holds decay, warm-up and updates; loading
    restores them, and a file without them raises KeyError when they are asked for"""
    ema = ModelEma(model, decay=0.98, warmup=False)
    with torch.no_grad():
        for p in ema.module.parameters():
            p.add_(1.0)
    plain, with_ema = str(tmp_path / "plain.tar"), str(tmp_path / "ema.tar")
    checkpoint.save_checkpoint(plain, model, config={"a": 1}, epoch=3)
    checkpoint.save_checkpoint(with_ema, model, config={"a": 1}, epoch=3, ema=ema)
    a = torch.load(plain, map_location="cpu", weights_only=False)
    b = torch.load(with_ema, map_location="cpu", weights_only=False)
    assert set(b) - set(a) == {"model_ema", "ema"} and set(a) <= set(b)
    assert list(a["model"].keys()) == list(b["model"].keys()) == list(b["model_ema"].keys())
    assert all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    assert all(b["model_ema"][k].dtype == b["model"][k].dtype for k in b["model"])
    k0 = next(k for k, v in model.named_parameters())
    assert torch.equal(b["model_ema"][k0], b["model"][k0] + 1.0)
    assert b["ema"] == {"decay": 0.98, "warmup": False, "updates": 0}
    other = ModelEma(model, decay=0.5)
    checkpoint.load_checkpoint(with_ema, model, ema=other)
    assert (other.decay, other.warmup, other.updates) == (0.98, False, 0)
    assert all(torch.equal(v, b["model_ema"][k]) for k, v in other.module.state_dict().items())
    with pytest.raises(KeyError):
        checkpoint.load_checkpoint(plain, model, ema=other)
    from mammo_clip_amd.breastclip.evaluator import Evaluator
    with pytest.raises(KeyError, match="model_ema"):
        Evaluator(ckpt_path=plain, use_ema=True, device="cpu")


def test_update_on_cpu_tensors_raises():
    m = _tiny()
    ema = ModelEma(m, decay=0.9)
    before = {k: v.clone() for k, v in ema.module.state_dict().items()}
    with pytest.raises(L.MammoClipHipError):
        ema.update(m)
    assert all(torch.equal(v, before[k]) for k, v in ema.module.state_dict().items()) and ema.updates == 0
    from mammo_clip_amd.breastclip.optimizer import AdamW
    m[0].weight.grad = torch.zeros_like(m[0].weight)
    with pytest.raises(L.MammoClipHipError):
        AdamW(list(m.parameters())).step(ema=ema)


def test_entry_points_check_their_arguments():
    """null lists, a decay outside (0, 1), a null count and negative sizes return non-zero before any launch"""
    lib = L.load()
    cnt = ctypes.c_longlong(0)                    # never dereferenced: every call below fails its checks first
    cp = ctypes.addressof(cnt)
    one = (ctypes.c_void_p * 1)(cp)
    n1, neg = (ctypes.c_longlong * 1)(4), (ctypes.c_longlong * 1)(-4)
    t = (L.AdamwTensor * 1)()
    t[0].param = t[0].grad = t[0].exp_avg = t[0].exp_avg_sq = cp
    t[0].numel = 4
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    def fails(status, why):                      # the check that is meant refused the call (its text names it): nothing ran
        return status != 0 and why in lib.mc_last_error()
    assert fails(lib.mc_ema_update(None, one, n1, 1, 0.9, 1, cp, None, None), b"ema_update: bad tensor lists")
    assert fails(lib.mc_ema_update(one, None, n1, 1, 0.9, 1, cp, None, None), b"ema_update: bad tensor lists")
    assert fails(lib.mc_ema_update(one, one, None, 1, 0.9, 1, cp, None, None), b"ema_update: bad tensor lists")
    assert fails(lib.mc_ema_update(one, one, n1, -1, 0.9, 1, cp, None, None), b"ema_update: bad tensor lists")
    assert fails(lib.mc_ema_update(one, one, neg, 1, 0.9, 1, cp, None, None), b"ema_update: negative size")
    assert fails(lib.mc_ema_update(one, one, n1, 1, 0.9, 1, None, None, None), b"ema_update: null update count")
    assert fails(lib.mc_ema_update(one, (ctypes.c_void_p * 1)(None), n1, 1, 0.9, 1, cp, None, None), b"ema_update: null tensor pointer")
    assert fails(lib.mc_adamw_step_ema(None, one, 1, *hyper, 0.9, 1, cp, None, None, None, None), b"adamw_step_ema: bad tensor or shadow list")
    assert fails(lib.mc_adamw_step_ema(t, None, 1, *hyper, 0.9, 1, cp, None, None, None, None), b"adamw_step_ema: bad tensor or shadow list")
    assert fails(lib.mc_adamw_step_ema(t, one, -1, *hyper, 0.9, 1, cp, None, None, None, None), b"adamw_step_ema: bad tensor or shadow list")
    assert fails(lib.mc_adamw_step_ema(t, one, 1, *hyper, 0.9, 1, None, None, None, None, None), b"adamw_step_ema: null update count")
    assert fails(lib.mc_adamw_step_ema(t, one, 1, *hyper, 0.9, 1, cp, None, cp, None, None), b"both null or both set")
    assert fails(lib.mc_adamw_step_ema(t, (ctypes.c_void_p * 1)(None), 1, *hyper, 0.9, 1, cp, None, None, None, None), b"null shadow pointer")
    t[0].numel = -4
    assert fails(lib.mc_adamw_step_ema(t, one, 1, *hyper, 0.9, 1, cp, None, None, None, None), b"adamw_step_ema: negative size")
    t[0].numel = 4
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        assert fails(lib.mc_ema_update(one, one, n1, 1, bad, 1, cp, None, None), b"ema_update: decay"), bad
        assert fails(lib.mc_adamw_step_ema(t, one, 1, *hyper, bad, 1, cp, None, None, None, None), b"adamw_step_ema: decay"), bad
    assert fails(lib.mc_ema_tick(None, None, None), b"ema_tick: null update count")
    assert cnt.value == 0


@pytest.mark.parametrize("fault", ["null", "oversized"])
def test_a_bad_tensor_past_the_first_pack_is_refused_before_any_launch(fault):
    """41 tensors, the first 40 (one full launch) well formed at dummy addresses, the 41st with a null pointer or with 2^30
    chunks: every entry point that walks the list returns MC_ERR_ARG with its own argument message, never a launch error.
    The whole list is checked before the first launch; the addresses are not memory."""
    lib = L.load()
    P, CHUNK = 0x10000, 16384
    t = (L.AdamwTensor * 41)()
    for a in t:
        a.param = a.grad = a.exp_avg = a.exp_avg_sq = P
        a.numel = 8
    shadows = (ctypes.c_void_p * 41)(*([P] * 41))
    if fault == "null":
        t[40].param = t[40].grad = t[40].exp_avg = t[40].exp_avg_sq = None
    else:
        t[40].numel = (1 << 30) * CHUNK
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    big = 1 << 40                                  # doubles of a norm workspace that is never written
    calls = [("adamw: null tensor pointer", lambda: lib.mc_adamw_step(t, 41, *hyper, None)),
             ("adamw: null tensor pointer", lambda: lib.mc_adamw_step_ema(t, shadows, 41, *hyper, 0.9, 1, P, None, None, None, None)),
             ("grads_unscale: null gradient pointer", lambda: lib.mc_grads_unscale(t, 41, 0.5, P, None)),
             ("grad_norm: bad tensor list", lambda: lib.mc_grad_norm(t, 41, P, big, 1.0, P, None)),
             ("grads_scale_dev: bad tensor list", lambda: lib.mc_grads_scale_dev(t, 41, P, None))]
    for null_msg, call in calls:
        want = null_msg if fault == "null" else ("adamw" if null_msg.startswith("adamw") else "grads_unscale") + ": tensor too large"
        assert call() == 1, want                    # MC_ERR_ARG; a launch that failed would return MC_ERR_LAUNCH = 2
        assert lib.mc_last_error().decode() == want
