"""SGD on the HIP optimizer step, the part that needs no GPU: the restatement of the rule (tests/_sgd_ref.py) against
``torch.optim.SGD`` in float64 within a bound counted from the rule, the host surface of ``breastclip.optimizer.SGD`` next to
``torch.optim.SGD`` (constructor, ``param_groups``, ``state_dict`` both ways, the factory, the refusal of CPU tensors) and the
argument checks of ``mc_sgd_step``.  The kernel's arithmetic is tested on the device in test_sgd_gpu.py."""
import copy
import ctypes
import os
import re

import pytest
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import lib as L
from mammo_clip_amd.breastclip.optimizer import SGD, AdamW, build_optimizer

import _sgd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = R.combos()
LR = 0.05


def _id(c):
    return "mu{momentum}-damp{dampening}-nest{nesterov:d}-wd{weight_decay}-max{maximize:d}".format(**c)


def test_combos_are_what_torch_accepts():
    """2 x 2 x 2 x 2 x 2 = 32 combinations; torch refuses nesterov without momentum or with dampening: 20 remain"""
    n_ok = 0
    for mu in (0.0, 0.9):
        for damp in (0.0, 0.5):
            for nest in (False, True):
                try:
                    torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=LR, momentum=mu, dampening=damp, nesterov=nest)
                    ok = True
                except ValueError:
                    ok = False
                assert ok == any(c["momentum"] == mu and c["dampening"] == damp and c["nesterov"] == nest for c in COMBOS)
                n_ok += 4 * ok
    assert n_ok == len(COMBOS) == 20


@pytest.mark.parametrize("combo", COMBOS, ids=_id)
def test_restatement_vs_torch_sgd_in_float64(combo):
    """a first step and two later ones, each from identical state (the fp32 result of the restatement so far): torch.optim.SGD in
    float64 on the same fp32-valued inputs -- the hyper-parameters as the fp32 values the kernel receives -- takes ONE step;
    |x32 - x64| <= k * 2^-24 * A * 1.01, k = 6 for the buffer and 10 for the parameter, A the float64 expression over absolute
    values.  The helper's own float64 values must be torch's (within 8 * 2^-53 * A: torch's float64 step rounds in other
    places), so that A belongs to what torch computes."""
    gen = torch.Generator().manual_seed(11)
    n = 4099
    p = torch.randn(n, generator=gen) * torch.logspace(-3, 3, n)
    buf = None
    h64 = {k: (float(R.f32(v)) if isinstance(v, float) else v) for k, v in combo.items()}
    worst = [0.0, 0.0]
    for step in range(3):
        g = torch.randn(n, generator=gen) * torch.logspace(2, -4, n)
        q = torch.nn.Parameter(p.double())
        q.grad = g.double()
        opt = torch.optim.SGD([q], lr=float(R.f32(LR)), foreach=False, **h64)
        if buf is not None:
            opt.state[q]["momentum_buffer"] = buf.double()
        opt.step()
        p64, b64, a_p, a_b = R.fp64_step(p, g, buf, lr=LR, **combo)
        assert bool(((p64 - q.detach()).abs() <= 8 * 2.0 ** -53 * a_p).all())
        p32, b32 = R.sgd_step(p, g, buf, lr=LR, **combo)
        assert p32.dtype == torch.float32
        err_p = (p32.double() - q.detach()).abs()
        worst[0] = max(worst[0], float((err_p / (R.U * a_p)).max()))
        assert bool((err_p <= R.K_P * R.U * a_p * 1.01).all()), (step, float((err_p / (R.U * a_p)).max()))
        if combo["momentum"] != 0:
            t64 = opt.state[q]["momentum_buffer"]
            assert bool(((b64 - t64).abs() <= 8 * 2.0 ** -53 * a_b).all())
            err_b = (b32.double() - t64).abs()
            worst[1] = max(worst[1], float((err_b / (R.U * a_b)).max()))
            assert bool((err_b <= R.K_BUF * R.U * a_b * 1.01).all()), (step, float((err_b / (R.U * a_b)).max()))
            if step == 0 and combo["weight_decay"] == 0:
                assert torch.equal(b32.double(), t64)              # the first step: buf = g', no dampening, nothing rounds
        else:
            assert b32 is None and b64 is None and "momentum_buffer" not in opt.state[q]
        p, buf = p32, b32
    print(f"{_id(combo)}: worst error in units of 2^-24 A: p {worst[0]:.2f} (bound 10), buf {worst[1]:.2f} (bound 6)")


def test_replay_skips_and_late_parameters():
    """Replay: a skipped step changes nothing and the next one is a first step; a tensor without a gradient stays out"""
    p = [torch.arange(4.0), torch.ones(3)]
    r = R.Replay(p, shadows=p, decay=0.9, lr=0.5, momentum=0.5)
    g = [torch.ones(4), torch.ones(3)]
    r.step(g, skipped=True)
    assert r.buf == [None, None] and r.updates == 0 and torch.equal(r.p[0], p[0]) and torch.equal(r.e[0], p[0])
    r.step([g[0], None])
    assert torch.equal(r.buf[0], g[0]) and r.buf[1] is None and torch.equal(r.p[0], p[0] - 0.5) and torch.equal(r.p[1], p[1])
    assert r.updates == 1 and torch.equal(r.e[0], p[0] + R.ema_weight(1, 0.9) * (r.p[0] - p[0]))
    r.step(g)
    assert torch.equal(r.buf[0], torch.full((4,), 1.5)) and torch.equal(r.buf[1], g[1]) and r.updates == 2


# ------------------------------------------------------------------------------------------------ host surface
def _params(n=2):
    return [torch.nn.Parameter(torch.randn(3, 2)) for _ in range(n)]


CTOR_CASES = [dict(), dict(lr=0.1), dict(lr=0.0), dict(lr=-1.0), dict(lr=torch.tensor(0.1)), dict(lr=torch.tensor([0.1, 0.2])),
              dict(momentum=0.9), dict(momentum=-0.1), dict(weight_decay=-1e-3), dict(weight_decay=1e-3, dampening=0.5),
              dict(nesterov=True), dict(nesterov=True, momentum=0.9), dict(nesterov=True, momentum=0.9, dampening=0.1),
              dict(maximize=True, momentum=0.5), dict(foreach=True), dict(fused=True, differentiable=True),
              dict(fused=True, foreach=True), dict(fused=False, foreach=True), dict(differentiable=True),
              dict(betas=(0.9, 0.99))]


@pytest.mark.parametrize("kw", CTOR_CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) or "defaults" for c in CTOR_CASES])
def test_constructor_is_torch_sgds(kw):
    """same acceptance, same exception type and text, same param_groups keys and values"""
    def make(cls):
        try:
            return cls(_params(), **kw)
        except (ValueError, RuntimeError, TypeError) as e:
            return e
    mine, ref = make(SGD), make(torch.optim.SGD)
    if isinstance(ref, Exception):
        assert type(mine) is type(ref)
        if not isinstance(ref, TypeError):                       # (a TypeError's text names the class)
            assert str(mine) == str(ref)
        return
    assert isinstance(mine, SGD) and isinstance(mine, torch.optim.Optimizer)
    assert len(mine.param_groups) == len(ref.param_groups) == 1
    a, b = mine.param_groups[0], ref.param_groups[0]
    assert list(a.keys()) == list(b.keys())
    assert all(a[k] == b[k] or (a[k] is b[k]) for k in a if k != "params")


def test_positional_arguments_and_group_overrides():
    mine = SGD([{"params": _params(1), "lr": 0.5}, {"params": _params(1), "momentum": 0.0}], 0.1, 0.9, 0.0, 1e-4, True)
    ref = torch.optim.SGD([{"params": _params(1), "lr": 0.5}, {"params": _params(1), "momentum": 0.0}], 0.1, 0.9, 0.0, 1e-4, True)
    for a, b in zip(mine.param_groups, ref.param_groups):
        assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in b.items() if k != "params"}
    with pytest.raises(TypeError):
        SGD(_params(), 0.1, 0.9, 0.0, 0.0, False, True)           # maximize is keyword-only, as in torch


def test_unstepped_state_dict_equals_torchs():
    ps = _params(3)
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    a, b = SGD(ps, **kw).state_dict(), torch.optim.SGD(ps, **kw).state_dict()
    assert a == b and a["state"] == {} and a["param_groups"][0]["params"] == [0, 1, 2]
    assert list(a["param_groups"][0].keys()) == list(b["param_groups"][0].keys())


def test_state_moves_both_ways_with_torch_sgd():
    """a torch.optim.SGD that has stepped -> load_state_dict into SGD -> state_dict() gives the same buffers and groups back, and
    torch.optim.SGD loads that again; a parameter torch has not stepped has no entry on either side"""
    ps = _params(3)
    kw = dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    ref = torch.optim.SGD(ps, **kw)
    for p in ps[:2]:
        p.grad = torch.randn_like(p)
    ref.step()
    sd = ref.state_dict()
    assert set(sd["state"]) == {0, 1}
    mine = SGD(ps, lr=7.0)
    mine.load_state_dict(sd)
    back = mine.state_dict()
    assert back["param_groups"] == sd["param_groups"] and set(back["state"]) == {0, 1}
    for i in (0, 1):
        assert set(back["state"][i]) == {"momentum_buffer"}
        assert torch.equal(back["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
    assert ps[2] not in mine.state and mine.param_groups[0]["lr"] == 0.1
    again = torch.optim.SGD(ps, lr=3.0)
    again.load_state_dict(copy.deepcopy(back))                   # (load_state_dict shares tensors of the same device)
    assert again.param_groups[0]["momentum"] == 0.9 and again.param_groups[0]["dampening"] == 0.1
    assert all(torch.equal(again.state[p]["momentum_buffer"], ref.state[p]["momentum_buffer"]) for p in ps[:2])
    before = [p.detach().clone() for p in ps]
    ref.step()
    after_ref = [p.detach().clone() for p in ps]
    with torch.no_grad():
        for p, v in zip(ps, before):
            p.copy_(v)
    again.step()
    assert all(torch.equal(p.detach(), v) for p, v in zip(ps, after_ref))


def test_build_optimizer_returns_the_hip_classes():
    m = torch.nn.Linear(3, 2)
    opt = build_optimizer(m, {"name": "SGD", "config": {"lr": 0.1, "momentum": 0.9, "nesterov": True}})
    assert type(opt) is SGD and hasattr(opt, "step_loss_scaled")
    assert opt.param_groups[0]["momentum"] == 0.9 and opt.param_groups[0]["nesterov"] is True
    assert opt.param_groups[0]["params"] == list(m.parameters())
    assert type(build_optimizer(m, {"name": "adamw", "config": {"lr": 0.1}})) is AdamW
    with pytest.raises(NotImplementedError):
        build_optimizer(m, {"name": "lamb", "config": {}})


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_step_on_cpu_parameters_raises(momentum):
    ps = _params()
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    opt = SGD(ps, lr=0.1, momentum=momentum)
    with pytest.raises(L.MammoClipHipError, match="SGD: parameters must be dense contiguous fp32 tensors on the GPU"):
        opt.step()
    assert all(torch.equal(p.detach(), v) for p, v in zip(ps, before))
    assert opt.state_dict()["state"] == {}
    half = [torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))]
    half[0].grad = torch.zeros_like(half[0])
    with pytest.raises(L.MammoClipHipError):
        SGD(half, lr=0.1).step()
    with pytest.raises(L.MammoClipHipError, match="grad_coef"):
        opt.step(grad_coef=torch.ones(1))


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_what_lib_binds():
    header = open(os.path.join(ROOT, "include", "mammoclip_hip.h")).read()
    m = re.search(r"\bint\s+mc_sgd_step\s*\(([^;]*)\)\s*;", header)
    assert m, "mc_sgd_step is declared in include/mammoclip_hip.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    argtypes, restype = L._SIGS["mc_sgd_step"]
    assert len(args) == len(argtypes) == 17 and restype is ctypes.c_int
    for a, t in zip(args, argtypes):
        want = (ctypes.c_double if a.startswith("double ") else ctypes.c_longlong if a.startswith("long long ") else
                ctypes.c_int if a.startswith("int ") else None)
        if want is not None:
            assert t is want, a
        else:
            assert "*" in a and t in (ctypes.c_void_p, ctypes.POINTER(L.AdamwTensor)), a
    assert "mc_sgd_step" in L.EXPORTS
    assert "optimizer/__init__.py:26-27" in header                # the reference call site it replaces
    assert hasattr(L.load(), "mc_sgd_step")
    f16 = os.path.join(os.path.dirname(L.LIB_PATH), "libmammoclip_hip_f16.so")
    assert hasattr(ctypes.CDLL(f16), "mc_sgd_step")


def test_entry_point_checks_its_arguments():
    """every bad call returns non-zero before any launch, with the message of the check that refused it"""
    lib = L.load()
    cnt = ctypes.c_longlong(0)                    # never dereferenced: every call below fails its checks first
    cp = ctypes.addressof(cnt)
    one = (ctypes.c_void_p * 1)(cp)
    t = (L.AdamwTensor * 1)()
    t[0].param = t[0].grad = t[0].exp_avg = cp
    t[0].numel = 4

    def call(tensors=t, shadows=None, n=1, lr=0.1, mu=0.9, damp=0.0, wd=0.0, nest=0, mx=0, step=1, decay=0.9, warmup=1, count=cp,
             coef=None, flag=None, skipped=None):
        return lib.mc_sgd_step(tensors, shadows, n, lr, mu, damp, wd, nest, mx, step, decay, warmup, count, coef, flag, skipped, None)

    def fails(status, why):
        return status != 0 and why in lib.mc_last_error()
    assert fails(call(tensors=None), b"sgd_step: bad tensor list")
    assert fails(call(n=-1), b"sgd_step: bad tensor list")
    assert fails(call(shadows=(ctypes.c_void_p * 1)(None)), b"sgd_step: null shadow pointer")
    assert fails(call(flag=cp), b"sgd_step: found_inf and skipped are both null or both set")
    assert fails(call(skipped=cp), b"sgd_step: found_inf and skipped are both null or both set")
    assert fails(call(nest=1, mu=0.0), b"sgd_step: nesterov requires a momentum and zero dampening")
    assert fails(call(nest=1, damp=0.5), b"sgd_step: nesterov requires a momentum and zero dampening")
    assert fails(call(lr=-0.1), b"sgd_step: negative or nan lr")
    assert fails(call(lr=float("nan")), b"sgd_step: negative or nan lr")
    assert fails(call(mu=-0.5), b"sgd_step: negative or nan momentum")
    assert fails(call(wd=-1e-3), b"sgd_step: negative or nan weight_decay")
    assert fails(call(step=0), b"sgd_step: step counts from 1")
    assert fails(call(shadows=one, count=None), b"sgd_step: null update count")
    for bad in (0.0, 1.0, -0.5, float("nan")):
        assert fails(call(shadows=one, decay=bad), b"sgd_step: decay"), bad
    t[0].numel = -4
    assert fails(call(), b"sgd_step: negative size")
    t[0].numel = 4
    t[0].exp_avg = None
    assert fails(call(), b"sgd_step: null tensor pointer")       # a momentum needs its buffer
    t[0].exp_avg, t[0].grad = cp, None
    assert fails(call(mu=0.0), b"sgd_step: null tensor pointer")
    t[0].grad, t[0].numel = cp, 0
    assert call(tensors=t, shadows=(ctypes.c_void_p * 1)(None)) == 0   # an empty tensor needs no pointers and launches nothing
    assert cnt.value == 0
