"""build_optimizer [ref: optimizer/__init__.py:10-32].  The reference's ``no_decay`` branch is dead code
(``getattr`` on a dict is always ``[]``), so weight decay applies to EVERY parameter incl. logit_scale / BN / LayerNorm;
that behaviour is kept.

``AdamW`` below is the hot loop's optimizer step: the same hyper-parameters, update rule
and ``state_dict()`` layout as ``torch.optim.AdamW`` (state per parameter: ``step``, ``exp_avg``, ``exp_avg_sq``), so
optimizer checkpoints move both ways [ref: trainer.py:215-237 stores ``optimizer.state_dict()``], with the update done
by one multi-tensor HIP kernel per 40 parameters (``mc_adamw_step``).

``SGD`` is the factory's other name [ref: optimizer/__init__.py:26-27]: ``torch.optim.SGD``'s arguments, checks, ``param_groups``
and ``state_dict()`` layout (``momentum_buffer`` per parameter) over ``mc_sgd_step``.  Both classes share ``_HipOptimizer``: the
launch plans, the step counts, the loss-scaled step, the EMA table and the bf16 weight images."""
import ctypes
import weakref
from typing import Dict

import torch
from torch import nn

from .. import lib as L


class _HipOptimizer(torch.optim.Optimizer):
    """What the HIP optimizers share.  A subclass says where a parameter's state lives (``_state_ptrs``, ``_init_state``), how
    applied step counts are written back to it (``_publish``) and which entry point one launch set calls (``_launcher``)."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._plans = {}          # group index -> host-side launch plan (pointer table, step counters)

    # ---- for the subclass
    def _state_ptrs(self, p, group):
        """(exp_avg, exp_avg_sq) slots of the tensor table as they are now (None: unused)"""
        raise NotImplementedError

    def _init_state(self, p, group):
        """create the state of ``p`` if it has none; the number of steps applied to it so far"""
        raise NotImplementedError

    def _publish(self, params, applied):
        """the applied step counts are being looked at: bring ``self.state`` up to date"""
        raise NotImplementedError

    def _launcher(self, group, grad_coef, ls, ema, stream):
        """-> f(tensor table, shadow table or None, number of tensors, step count) that launches one set"""
        raise NotImplementedError

    # The hot loop counts steps in Python ints and writes them back only when the state is looked at (state_dict) -- 700 tiny
    # CPU tensor updates per step are host time the small configurations cannot hide.
    def _sync_steps(self):
        # loss-scaled steps (step_loss_scaled): the host counts ATTEMPTED steps, the device counts the skipped ones
        skipped = int(self._ls_skipped.item()) if getattr(self, "_ls_skipped", None) is not None else 0
        for plan in self._plans.values():
            self._publish(plan["params"], [max(t - skipped, 0) for t in plan["steps"]])
        return skipped

    def _fold_skipped(self):
        """make the host counts the APPLIED counts and clear the device counter of skipped steps (before plans are rebuilt
        from the state: a rebuilt plan must not subtract the same skips again)"""
        skipped = self._sync_steps()
        if getattr(self, "_ls_skipped", None) is not None:
            for plan in self._plans.values():
                plan["steps"][:] = [max(t - skipped, 0) for t in plan["steps"]]
            self._ls_skipped.zero_()

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def _plan(self, gi, group):
        params = [p for p in group["params"] if p.grad is not None]
        plan = self._plans.get(gi)
        if plan is not None and len(plan["params"]) == len(params) and all(a is b for a, b in zip(plan["params"], params)):
            # the plan caches raw device pointers: it is only valid while every parameter / state tensor still lives
            # where it did (model.to(), p.data = ..., a state moved or replaced by external code all change data_ptr)
            if all((p.data_ptr(),) + self._state_ptrs(p, group) == ptrs for p, ptrs in zip(params, plan["ptrs"])):
                return plan
        if getattr(self, "_ls_skipped", None) is not None:
            # a plan is created or rebuilt while the device counts skipped steps: fold them into the host counts FIRST -- the
            # new plan reads the state (applied counts) and must not have the same skips subtracted again, and a
            # group planned for the first time after some skips must not inherit them
            self._fold_skipped()
        else:
            # plain steps: the counts live in the plan that is being replaced; the state is only as fresh as the
            # last state_dict() call, and a rebuilt plan (the set of parameters with a gradient changed) reads it below
            self._sync_steps()
        steps = []
        arr = (L.AdamwTensor * max(len(params), 1))()
        for i, p in enumerate(params):
            if not p.is_cuda or p.dtype != torch.float32 or p.grad.is_sparse or not p.is_contiguous():
                raise L.MammoClipHipError(f"{type(self).__name__}: parameters must be dense contiguous fp32 tensors on the GPU "
                                          "(the HIP kernel is the only path)")
            steps.append(self._init_state(p, group))
            a = arr[i]
            a.param, a.numel = p.data_ptr(), p.numel()
            a.exp_avg, a.exp_avg_sq = self._state_ptrs(p, group)
        ptrs = [(a.param, a.exp_avg, a.exp_avg_sq) for a in arr[:len(params)]]
        plan = {"params": params, "steps": steps, "arr": arr, "gen": -1, "images": {}, "keep": [], "ptrs": ptrs}
        self._plans[gi] = plan
        return plan

    def _ema_table(self, plan, ema):
        """the shadow pointers of ``plan``'s parameters, parallel to its tensor table; cached with the plan and validated like
        its other raw pointers (a shadow moved or replaced changes data_ptr)"""
        tab = plan.get("ema")
        if tab is not None and tab["of"]() is ema and len(tab["shadows"]) == len(plan["params"]) and \
                all(e.data_ptr() == ptr for e, ptr in zip(tab["shadows"], tab["ptrs"])):
            return tab
        shadows = ema.shadows_for(plan["params"])
        for p, e in zip(plan["params"], shadows):
            if e.numel() != p.numel() or e.data_ptr() == p.data_ptr():
                raise L.MammoClipHipError(f"{type(self).__name__}: an EMA shadow must be a tensor of its own with the parameter's size")
        ptrs = [e.data_ptr() for e in shadows]
        tab = plan["ema"] = {"of": weakref.ref(ema), "shadows": shadows, "ptrs": ptrs,
                             "arr": (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)}
        return tab

    @torch.no_grad()
    def step_loss_scaled(self, scaler, grad_coef=None, ema=None):
        """``step()`` under an ``engine.LossScaler`` without a host sync: the kernel reads the scaler's non-finite flag and
        does nothing on a bad step (GradScaler.step() would not call optimizer.step()); what depends on the step index (AdamW's
        bias corrections, SGD's first step) uses the
        number of APPLIED steps = attempted steps (counted on the host) - skipped steps (counted on the device, in a tensor
        this optimizer owns: it survives a change of scaler).  Returns that counter for ``scaler.update``.
        ``grad_coef``, ``ema``: as in ``step``; on a skipped step the shadows stay as they are, like the parameters."""
        dev = self.param_groups[0]["params"][0].device
        if getattr(self, "_ls_skipped", None) is None or self._ls_skipped.device != dev:
            self._fold_skipped()                           # (a counter on another device: fold it into the host counts)
            self._ls_skipped = torch.zeros(1, dtype=torch.float32, device=dev)
        st = scaler.state(dev)
        self._ls = (st.data_ptr() + 4 * scaler._FLAG, self._ls_skipped.data_ptr())
        try:
            self.step(grad_coef=grad_coef, ema=ema)
        finally:
            self._ls = None
        return self._ls_skipped

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}
        self._ls_skipped = None

    @torch.no_grad()
    def step(self, closure=None, grad_coef=None, ema=None):
        """``grad_coef``: a 1-element fp32 device tensor (the clip coefficient of ``ops.grad_norm_coef``); every gradient is
        multiplied by it as the kernel loads it, ``p.grad`` itself is left as it is.
        ``ema``: a ``mammo_clip_amd.ema.ModelEma`` of the model these parameters belong to: the pass
        also moves the shadow of every element it updates; ``ema.update(model)`` afterwards does the tensors this pass
        did not cover and advances the count of updates."""
        loss = None
        if grad_coef is not None and not (torch.is_tensor(grad_coef) and grad_coef.is_cuda and grad_coef.dtype == torch.float32
                                          and grad_coef.numel() >= 1):
            raise L.MammoClipHipError(f"{type(self).__name__}: grad_coef must be an fp32 tensor on the GPU (the HIP kernel is the only path)")
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from .. import ops
        if getattr(self, "_ls", None) is None and getattr(self, "_ls_skipped", None) is not None:
            # a plain step() after loss-scaled ones: the kernel is handed the APPLIED count (no device counter in this call)
            self._fold_skipped()
            self._ls_skipped = None
        for gi, group in enumerate(self.param_groups):
            plan = self._plan(gi, group)
            params, arr, steps = plan["params"], plan["arr"], plan["steps"]
            if not params:
                continue
            if plan["gen"] != ops.cache_generation():          # bf16 images the kernel keeps current (see ops._cached)
                plan["images"] = ops.cached_cast_images(params)
                plan["gen"] = ops.cache_generation()
                for i, p in enumerate(params):
                    im = plan["images"].get(id(p))
                    arr[i].bf16_image = im[1].data_ptr() if im is not None else None
            keep = plan["keep"] = []
            for i, p in enumerate(params):
                g = p.grad
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                arr[i].grad = g.data_ptr()
                steps[i] += 1
            stream = torch.cuda.current_stream().cuda_stream
            tab = self._ema_table(plan, ema) if ema is not None else None
            launch = self._launcher(group, grad_coef, getattr(self, "_ls", None), ema if tab is not None else None, stream)
            if min(steps) == max(steps):
                launch(arr, tab["arr"] if tab else None, len(params), steps[0])
            else:                                             # parameters that joined later: one launch set per step count
                for t in sorted(set(steps)):
                    idx = [i for i, s_ in enumerate(steps) if s_ == t]
                    sub = (L.AdamwTensor * len(idx))(*[arr[i] for i in idx])
                    ssub = (ctypes.c_void_p * len(idx))(*[tab["ptrs"][i] for i in idx]) if tab else None
                    launch(sub, ssub, len(idx), t)
            if tab is not None:
                ema.mark_covered(params, tab["shadows"])       # (bumps the shadows' version counters, as below)
            # the kernel wrote through raw pointers: tell autograd (and the derived-weight-image cache in ops.py,
            # which keys on the version counter) that these tensors changed in place
            torch.autograd.graph.increment_version(params)
            ops.stamp_cast_images(plan["images"])              # ... and that the images it rewrote are current
            self._stepped(plan)
        return loss

    def _stepped(self, plan):
        """after the launches of one group"""


class AdamW(_HipOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **unused):
        if amsgrad:
            raise NotImplementedError("amsgrad is not used by the reference configs")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))

    # The per-parameter ``state["step"]`` tensors of torch.optim.AdamW are kept (see _HipOptimizer._sync_steps)
    def _publish(self, params, applied):
        for p, t in zip(params, applied):
            self.state[p]["step"].fill_(float(t))

    def _state_ptrs(self, p, group):
        st = self.state[p]
        return st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()

    def _init_state(self, p, group):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return int(st["step"])

    def _launcher(self, group, grad_coef, ls, ema, stream):
        """``mc_adamw_step``; with a loss scale ``_ls``, with ``grad_coef`` ``_clip``, with ``ema`` ``mc_adamw_step_ema``"""
        b1, b2 = group["betas"]
        hyper = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
        if ema is not None:
            # (the table of shadow pointers goes in front of the count; every optional pointer may be None)
            entry = "mc_adamw_step_ema"
            tail = (float(ema.decay), int(ema.warmup), ema.count_ptr(), grad_coef.data_ptr() if grad_coef is not None else None,
                    ls[0] if ls else None, ls[1] if ls else None, stream)
        elif grad_coef is not None:
            entry, tail = "mc_adamw_step_clip", (grad_coef.data_ptr(), ls[0] if ls else None, ls[1] if ls else None, stream)
        else:
            entry, tail = ("mc_adamw_step_ls", (ls[0], ls[1], stream)) if ls else ("mc_adamw_step", (stream,))

        def launch(arr, shadows, n, t):
            L.call(entry, arr, *((shadows,) if ema is not None else ()), n, *hyper, t, *tail)
        return launch


class SGD(_HipOptimizer):
    """``torch.optim.SGD`` over ``mc_sgd_step`` (the rule is in include/mammoclip_hip.h).  ``state[p]`` holds ``momentum_buffer``
    once a step has been APPLIED to ``p`` with a momentum, and nothing before: a buffer the launch plan had to allocate ahead of
    a step that may be skipped waits in ``_pending``.  The kernel's first-step decision needs no more than "has a buffer": the
    host count of a parameter starts at 1 with a published buffer and at 0 without."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._pending = {}        # parameter -> momentum buffer no applied step has written yet
        # (foreach / differentiable / fused: torch's group keys, kept for checkpoints that move both ways; there is one path here)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused))
        if fused:
            if differentiable:
                raise RuntimeError("`fused` does not support `differentiable`")
            if foreach:
                raise RuntimeError("`fused` and `foreach` cannot be `True` together.")

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("nesterov", False)
            group.setdefault("maximize", False)
            group.setdefault("foreach", None)
            group.setdefault("differentiable", False)
            group.setdefault("fused", False)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._pending = {}

    def _buffer(self, p):
        st = self.state.get(p)                             # (never ``self.state[p]``: torch's SGD has no entry before a step)
        buf = st.get("momentum_buffer") if st else None
        return buf if buf is not None else self._pending.get(p)

    def _publish(self, params, applied):
        for p, t in zip(params, applied):
            if t >= 1 and p in self._pending:
                self.state[p]["momentum_buffer"] = self._pending.pop(p)

    def _state_ptrs(self, p, group):
        buf = self._buffer(p) if group["momentum"] != 0 else None
        return (buf.data_ptr() if buf is not None else None), None

    def _init_state(self, p, group):
        if group["momentum"] == 0:
            return 0
        buf = self._buffer(p)
        if buf is None:
            buf = self._pending[p] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif not buf.is_cuda or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.numel() != p.numel():
            raise L.MammoClipHipError("SGD: momentum buffers must be dense contiguous fp32 tensors on the GPU "
                                      "(the HIP kernel is the only path)")
        return 0 if p in self._pending else 1

    def _launcher(self, group, grad_coef, ls, ema, stream):
        hyper = (float(group["lr"]), float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]),
                 int(bool(group["nesterov"])), int(bool(group["maximize"])))
        tail = ((float(ema.decay), int(ema.warmup), ema.count_ptr()) if ema is not None else (0.0, 0, None)) + \
               (grad_coef.data_ptr() if grad_coef is not None else None, ls[0] if ls else None, ls[1] if ls else None, stream)

        def launch(arr, shadows, n, t):
            L.call("mc_sgd_step", arr, shadows if ema is not None else None, n, *hyper, t, *tail)
        return launch

    def _stepped(self, plan):
        # plain steps are applied steps: the buffers they wrote are state from now on.  Under a loss scale only the device
        # knows; state_dict() and a plan rebuild read its counter then (_sync_steps).
        if self._pending and getattr(self, "_ls", None) is None:
            self._publish(plan["params"], plan["steps"])


def build_optimizer(model: nn.Module, optim_config: Dict):
    name = optim_config["name"].lower()
    params = list(model.parameters())
    if name == "sgd":
        return SGD(params, **optim_config["config"])        # HIP kernel only, like AdamW
    if name == "adamw":
        return AdamW(params, **optim_config["config"])      # HIP kernel only: .step() raises on CPU parameters
    raise NotImplementedError(f"Not implemented optimizer : {name}")
