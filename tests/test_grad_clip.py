"""Gradient-norm clipping, the part that needs no GPU: argument checks of the five C entry points (they run before any
launch), the workspace arithmetic of mc_grad_norm_partials, and the Python-side refusals."""
import math

import pytest
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import engine, lib as L, ops

CHUNK = 16384
HYPER = (3e-3, 0.9, 0.999, 1e-8, 0.05)
INF = float("inf")


def _table(numels, grad=0x1000):
    arr = (L.AdamwTensor * max(len(numels), 1))()
    for a, n in zip(arr, numels):
        a.grad, a.numel = grad, n              # the pointer is never followed: every call below is refused before a launch
    return arr


def _refused(lib, name, *args):
    assert getattr(lib, name)(*args) != 0, name
    msg = lib.mc_last_error().decode()
    assert name[3:] in msg, (name, msg)         # "mc_grad_norm" names itself as "grad_norm: ..."
    return msg


def test_grad_norm_partials_arithmetic():
    lib = L.load()
    for n, want in [(0, 0), (1, 1), (CHUNK, 1), (CHUNK + 1, 2), (2 * CHUNK + 3, 3)]:
        assert lib.mc_grad_norm_partials(_table([n]), 1) == want, n
    assert lib.mc_grad_norm_partials(_table([5, 0, CHUNK + 1, 0, 2 * CHUNK + 3]), 5) == 1 + 2 + 3
    assert lib.mc_grad_norm_partials(None, 0) == 0
    assert lib.mc_grad_norm_partials(_table([5, -1, 7]), 3) == -1 and b"grad_norm_partials" in lib.mc_last_error()
    assert lib.mc_grad_norm_partials(None, 2) == -1 and b"grad_norm_partials" in lib.mc_last_error()
    assert lib.mc_grad_norm_partials(_table([5]), -1) == -1 and b"grad_norm_partials" in lib.mc_last_error()
    assert lib.mc_grad_norm_partials(_table([5], grad=None), 1) == 1          # host arithmetic: no pointer is looked at


def test_grad_norm_argument_validation_without_gpu():
    lib = L.load()
    arr, n, P = _table([5, CHUNK + 1]), 2, 0x2000                   # needs 3 doubles
    for max_norm in (0.0, -1.0, float("nan"), -INF):
        assert "max_norm" in _refused(lib, "mc_grad_norm", arr, n, P, 3, max_norm, P, None)
        assert "max_norm" in _refused(lib, "mc_grads_unscale_norm_dev", arr, n, P, P, P, 3, max_norm, P, None)
    assert "workspace" in _refused(lib, "mc_grad_norm", arr, n, P, 2, 1.0, P, None)
    assert "workspace" in _refused(lib, "mc_grad_norm", arr, n, None, 3, 1.0, P, None)
    _refused(lib, "mc_grad_norm", arr, n, P, 3, 1.0, None, None)
    _refused(lib, "mc_grad_norm", None, 2, P, 3, 1.0, P, None)
    _refused(lib, "mc_grad_norm", _table([5, -2]), 2, P, 3, 1.0, P, None)
    _refused(lib, "mc_grad_norm", _table([5, 3], grad=None), 2, P, 3, 1.0, P, None)
    assert "workspace" in _refused(lib, "mc_grads_unscale_norm_dev", arr, n, P, P, P, 2, INF, P, None)
    assert "workspace" in _refused(lib, "mc_grads_unscale_norm_dev", arr, n, P, P, None, 3, INF, P, None)
    _refused(lib, "mc_grads_unscale_norm_dev", arr, n, None, P, P, 3, 1.0, P, None)
    _refused(lib, "mc_grads_unscale_norm_dev", arr, n, P, None, P, 3, 1.0, P, None)
    _refused(lib, "mc_grads_unscale_norm_dev", arr, n, P, P, P, 3, 1.0, None, None)
    _refused(lib, "mc_grads_unscale_norm_dev", _table([-5]), 1, P, P, P, 3, 1.0, P, None)
    _refused(lib, "mc_grads_scale_dev", arr, n, None, None)
    _refused(lib, "mc_grads_scale_dev", None, 1, P, None)
    _refused(lib, "mc_grads_scale_dev", _table([4], grad=None), 1, P, None)
    _refused(lib, "mc_adamw_step_clip", arr, n, *HYPER, 1, None, None, None, None)
    _refused(lib, "mc_adamw_step_clip", arr, n, *HYPER, 1, P, P, None, None)
    _refused(lib, "mc_adamw_step_clip", arr, n, *HYPER, 1, P, None, P, None)
    with pytest.raises(L.MammoClipHipError, match="grad_norm"):
        L.call("mc_grad_norm", arr, n, P, 3, 0.0, P, None)


def test_trainer_refuses_a_bad_max_grad_norm():
    for bad in (0, 0.0, -1, -1.0, float("nan"), -INF):
        with pytest.raises(ValueError, match="max_grad_norm"):
            engine.Trainer(torch.nn.Linear(2, 2), None, None, max_grad_norm=bad)
    assert engine.Trainer(torch.nn.Linear(2, 2), None, None).max_grad_norm is None
    assert engine.Trainer(torch.nn.Linear(2, 2), None, None, max_grad_norm=2).max_grad_norm == 2.0
    assert math.isinf(engine.Trainer(torch.nn.Linear(2, 2), None, None, max_grad_norm=INF).max_grad_norm)


def test_clip_grad_norm_has_no_cpu_fallback():
    p = torch.nn.Parameter(torch.ones(7))
    p.grad = torch.full((7,), 2.0)
    for call in (lambda: ops.clip_grad_norm_([p], 1.0), lambda: ops.clip_grad_norm_(p, 1.0), lambda: ops.grad_norm([p]),
                 lambda: ops.grads_scale_([p], torch.ones(1))):
        with pytest.raises(L.MammoClipHipError, match="no CPU fallback"):
            call()
    assert torch.equal(p.grad, torch.full((7,), 2.0))
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            ops.clip_grad_norm_([p], bad)
    # the gradient must be dense contiguous fp32, refused the way LossScaler refuses it -- before any device is looked at
    d = torch.nn.Parameter(torch.ones(7, dtype=torch.float64))
    d.grad = torch.full((7,), 2.0, dtype=torch.float64)
    with pytest.raises(L.MammoClipHipError, match="dense contiguous fp32"):
        ops.clip_grad_norm_([d], 1.0)
    q = torch.nn.Parameter(torch.ones(4, 6))
    q.grad = torch.ones(6, 4).t()
    with pytest.raises(L.MammoClipHipError, match="dense contiguous fp32"):
        ops.grad_norm([q])
    assert ops.grad_norm([torch.nn.Parameter(torch.ones(3))]).item() == 0.0      # no gradients at all: torch's tensor(0.)
    from mammo_clip_amd.breastclip.optimizer import AdamW
    with pytest.raises(L.MammoClipHipError, match="grad_coef"):
        AdamW([p]).step(grad_coef=torch.ones(1))
