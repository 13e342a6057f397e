"""Exponential moving average of the weights: a shadow model kept by the optimizer step, with no host sync.

CONTRACT (include/mammoclip_hip.h).  For every floating tensor of ``model.state_dict()``, parameters
and buffers alike, there is an fp32 shadow ``e``; with ``p`` the tensor's value after the optimizer step, one applied update
is three separately rounded fp32 operations, never fused::

    s = p - e;   t = w * s;   e = e + t          w = float32(1.0 - d_k)

``d_k = min(decay, (1.0 + k) / (10.0 + k))`` with warm-up, ``decay`` without, in double; ``k = 1, 2, ...`` counts the applied
updates including this one.  Integer buffers (``num_batches_tracked``) are copied.  A step the loss scaler skips changes no
shadow and does not advance ``k``: the count is a device integer this object owns, every launch of an update reads it and a
last one-thread launch advances it unless the scaler's non-finite flag is set -- so an update has to be complete before
``LossScaler.update`` clears that flag.  The host reads the count only when asked (``updates``, ``state_dict()``).

Two routes, one arithmetic: ``AdamW.step(ema=)`` / ``step_loss_scaled(ema=)`` (and ``SGD``'s) fold the shadows of the parameters they
update into the optimizer pass itself (``mc_adamw_step_ema``, ``mc_sgd_step``: the updated parameter is still in registers) and ``update(model)``
does the rest -- buffers, parameters the pass did not cover, everything under another optimizer (``mc_ema_update``) -- then
advances the count (``mc_ema_tick``).  There is no CPU fallback: on CPU tensors ``update`` raises, as ``AdamW`` does."""
import copy
import ctypes as C
import struct
import weakref

import torch

from . import lib as L


class ModelEma:
    def __init__(self, model, decay=0.9999, warmup=True):
        decay = float(decay)
        if not 0.0 < decay < 1.0:                                   # (false for nan)
            raise ValueError(f"ModelEma: decay must lie strictly between 0 and 1, got {decay}")
        if not isinstance(model, torch.nn.Module):
            raise TypeError("ModelEma: model must be a torch.nn.Module")
        self.decay, self.warmup = decay, bool(warmup)
        # ``module``: a second module instance whose parameter and buffer storages ARE the shadows.  ``engine.validate`` and
        # ``Evaluator(model=ema.module)`` take it as the model it is.
        self.module = copy.deepcopy(model)
        self.module.eval()
        for t in list(self.module.parameters()) + list(self.module.buffers()):
            if t.is_floating_point() and t.dtype != torch.float32:
                t.data = t.data.float()
        for p in self.module.parameters():
            p.requires_grad_(False)
            p.grad = None
        dev = next((t.device for t in self.module.parameters()), torch.device("cpu"))
        self._count = torch.zeros(1, dtype=torch.int64, device=dev)      # applied updates (lives with the shadows)
        self._model_ref = None       # weak reference to the model the pairing below was made for
        self._floats = []            # (name, source tensor, shadow) of every floating state tensor
        self._ints = []              # the same for the integer buffers
        self._shadow_of = {}         # id(source parameter) -> (weak reference to it, shadow): AdamW's route to the shadows
        self._int_flat = None        # one flat int64 tensor behind all integer shadows: their copy is one launch
        self._int_ptrs = []          # where each integer shadow lived when it was made a view of it
        self._covered = {}           # id(source parameter) -> shadow, folded into an optimizer pass since the last update()
        self._plans = {}             # frozenset(covered ids) -> launch plan of the stand-alone pass
        self.bind(model)

    # ---------------------------------------------------------------------------------------------- weight
    def decay_at(self, k):
        """d_k of the k-th applied update (k = 1, 2, ...), a double"""
        k = int(k)
        if k < 1:
            raise ValueError("decay_at: updates are counted from 1")
        return min(self.decay, (1.0 + k) / (10.0 + k)) if self.warmup else self.decay

    def weight_at(self, k):
        """w of the k-th applied update: 1.0 - d_k rounded to fp32 (what the kernels multiply by)"""
        return struct.unpack("f", struct.pack("f", 1.0 - self.decay_at(k)))[0]

    @property
    def updates(self):
        """applied updates so far (reads the device: synchronises)"""
        return int(self._count.item())

    # ---------------------------------------------------------------------------------------------- pairing with a model
    @staticmethod
    def _state_tensors(module):
        """name -> tensor for every entry of ``state_dict()`` (the tensors themselves, not detached copies)"""
        out = dict(module.named_parameters(remove_duplicate=False))
        out.update(dict(module.named_buffers(remove_duplicate=False)))
        keys = list(module.state_dict().keys())
        return {k: out[k] for k in keys}

    def bind(self, model):
        """pair the shadows with the tensors of ``model`` (an instance with the averaged module's state_dict layout); done by
        the constructor, by ``update`` for whatever model it is given, and by ``engine.Trainer`` for the one it trains"""
        if self._model_ref is not None and self._model_ref() is model:
            return
        src, dst = self._state_tensors(model), self._state_tensors(self.module)
        if list(src) != list(dst):
            raise ValueError("ModelEma: the model's state_dict does not have the keys of the averaged module")
        self._floats, self._ints, self._shadow_of = [], [], {}
        for k in dst:
            s, e = src[k], dst[k]
            if tuple(s.shape) != tuple(e.shape):
                raise ValueError(f"ModelEma: {k} has shape {tuple(s.shape)}, the averaged module {tuple(e.shape)}")
            if e.is_floating_point():
                self._floats.append((k, s, e))
                self._shadow_of[id(s)] = (weakref.ref(s), e)
            else:
                self._ints.append((k, s, e))
        self._model_ref = weakref.ref(model)
        self._plans, self._covered = {}, {}

    def _to_device(self, dev):
        """the shadows follow the model to its device (a model moved after this object was built).  Module.to() replaces the
        buffer objects, so the pairing is made again."""
        if self._count.device != dev:
            model = self._model_ref() if self._model_ref is not None else None
            self.module.to(dev)
            self._count = self._count.to(dev)
            self._int_flat, self._model_ref = None, None
            if model is not None:
                self.bind(model)

    def shadows_for(self, params):
        """the shadows of ``params`` (parameters of the bound model) -- what ``AdamW.step(ema=)`` hands the kernel"""
        params = list(params)
        if params:
            self._to_device(params[0].device)
        out = []
        for p in params:
            hit = self._shadow_of.get(id(p))
            if hit is None or hit[0]() is not p:
                raise L.MammoClipHipError("ModelEma: the optimizer holds a parameter that is not one of the averaged model's")
            e = hit[1]
            if not e.is_cuda or e.device != p.device or e.dtype != torch.float32 or not e.is_contiguous():
                raise L.MammoClipHipError("ModelEma: shadows must be dense contiguous fp32 tensors on the parameters' GPU")
            out.append(e)
        return out

    def count_ptr(self):
        return self._count.data_ptr()

    def mark_covered(self, params, shadows):
        """``AdamW.step(ema=)`` has updated these shadows in its own pass: the next ``update()`` leaves them out.  Their version
        counters move like the parameters' (the kernel wrote through raw pointers): cached weight images of ``module`` rebuild."""
        for p, e in zip(params, shadows):
            self._covered[id(p)] = e
        torch.autograd.graph.increment_version(list(shadows))

    # ---------------------------------------------------------------------------------------------- the stand-alone pass
    def _plan(self, covered):
        key = frozenset(covered)
        plan = self._plans.get(key)
        if plan is not None and all(s.data_ptr() == a and e.data_ptr() == b for (s, e), (a, b) in zip(plan["pairs"], plan["ptrs"])):
            return plan
        pairs = [(s, e) for _k, s, e in self._floats if id(s) not in key]
        for s, e in pairs:
            if not (s.is_cuda and e.is_cuda and s.device == e.device and s.dtype == torch.float32 and e.dtype == torch.float32
                    and s.is_contiguous() and e.is_contiguous()):
                raise L.MammoClipHipError("ModelEma: model tensors and shadows must be dense contiguous fp32 tensors on one GPU "
                                          "(the HIP kernel is the only path)")
        n = max(len(pairs), 1)
        ptrs = [(s.data_ptr(), e.data_ptr()) for s, e in pairs]
        plan = {"pairs": pairs, "ptrs": ptrs, "n": len(pairs),
                "e": (C.c_void_p * n)(*[b for _a, b in ptrs]), "p": (C.c_void_p * n)(*[a for a, _b in ptrs]),
                "numel": (C.c_longlong * n)(*[e.numel() for _s, e in pairs]), "shadows": [e for _s, e in pairs]}
        if len(self._plans) > 8:
            self._plans.clear()
        self._plans[key] = plan
        return plan

    def _copy_ints(self, found_inf):
        """integer buffers are copied: one gather of the sources, one (conditional, under a scaler) copy into the flat tensor
        every integer shadow is a view of"""
        if not self._ints:
            return
        flat = self._int_flat
        if flat is None or any(e.data_ptr() != ptr for (_k, _s, e), ptr in zip(self._ints, self._int_ptrs)):
            dev = self._count.device
            if any(e.dtype != torch.int64 or s.dtype != torch.int64 for _k, s, e in self._ints):
                raise L.MammoClipHipError("ModelEma: integer buffers must be int64")
            flat = torch.cat([e.detach().reshape(-1).to(dev) for _k, _s, e in self._ints])
            off, self._int_ptrs = 0, []
            for _k, _s, e in self._ints:
                e.data = flat[off:off + e.numel()].view(e.shape)
                off += e.numel()
                self._int_ptrs.append(e.data_ptr())
            self._int_flat = flat
        new = torch.cat([s.detach().reshape(-1) for _k, s, _e in self._ints])
        if found_inf is not None:
            new = torch.where(found_inf != 0, flat, new)
        flat.copy_(new)

    @torch.no_grad()
    def update(self, model, found_inf=None):
        """One update of every shadow that an optimizer pass (``AdamW.step(ema=)``) has not already made since the last call --
        with no such pass: the stand-alone path over everything -- then the count moves on.  ``found_inf``: the loss scaler's
        non-finite flag, a 1-element fp32 device tensor; while it is set nothing changes and the count stays."""
        self.bind(model)
        first = next((s for _k, s, _e in self._floats + self._ints), None)
        if first is None:
            return
        if not first.is_cuda:
            raise L.MammoClipHipError("ModelEma.update: the model is not on the GPU (the HIP kernel is the only path)")
        self._to_device(first.device)
        if found_inf is not None and not (torch.is_tensor(found_inf) and found_inf.is_cuda and found_inf.dtype == torch.float32
                                          and found_inf.numel() >= 1):
            raise L.MammoClipHipError("ModelEma.update: found_inf must be an fp32 tensor on the GPU")
        covered, self._covered = self._covered, {}
        plan = self._plan(covered)
        flag = found_inf.data_ptr() if found_inf is not None else None
        stream = torch.cuda.current_stream().cuda_stream
        if plan["n"]:
            L.call("mc_ema_update", plan["e"], plan["p"], plan["numel"], plan["n"], self.decay, int(self.warmup),
                   self._count.data_ptr(), flag, stream)
            # the kernel wrote through raw pointers: cached weight images of ``module`` (ops.py keys on the version) rebuild
            torch.autograd.graph.increment_version(plan["shadows"])
        self._copy_ints(found_inf)
        L.call("mc_ema_tick", self._count.data_ptr(), flag, stream)

    # ---------------------------------------------------------------------------------------------- state
    def state_dict(self):
        """{"module": the shadows in the model's key layout, on the CPU, "decay", "warmup", "updates"}"""
        return {"module": {k: v.detach().to("cpu") for k, v in self.module.state_dict().items()},
                "decay": self.decay, "warmup": self.warmup, "updates": self.updates}

    def load_state_dict(self, sd):
        decay = float(sd["decay"])
        if not 0.0 < decay < 1.0:
            raise ValueError(f"ModelEma: decay must lie strictly between 0 and 1, got {decay}")
        mod = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd["module"].items()}
        self.module.load_state_dict(mod, strict=True)           # in place: storages (and cached pointers) stay, versions move
        self.decay, self.warmup = decay, bool(sd["warmup"])
        self._count.fill_(int(sd["updates"]))
        self._covered = {}
