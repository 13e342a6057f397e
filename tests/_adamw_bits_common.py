"""Shared by tests/test_adamw_bits_gpu.py and tests/golden/make_golden_adamw_bits.py: the cases whose bits the fixture
tests/golden/adamw_bits.json holds, and the digest of one array.

Inputs are ``AdamCase`` of tests/test_ema_gpu.py as it stands (its SIZES with the holes, HYPER, CPU-generator normals, seed
200; every third tensor has a 16-bit image), in both layouts.  Each case takes two steps of one entry point without EMA:

    step    mc_adamw_step, host steps 1 and 2
    clip    mc_adamw_step_clip with a device coefficient of 0.1, host steps 1 and 2
    ls      mc_adamw_step_ls with the non-finite flag at 0 and a device counter of 1 skipped step, host steps 3 and 4
            (applied steps 2 and 3: the bias corrections are derived on the device)

A digest is the first 12 hex digits of the sha256 of an array's little-endian bit image.  There is one per non-empty tensor and
per array (parameter, exp_avg, exp_avg_sq, image where the tensor has one), under a key that names the tensor's position and
size, so that a mismatch names the loop body that moved."""
import hashlib
import os
import sys

import torch

from mammo_clip_amd import lib as L, ops
from test_ema_gpu import DEV, LAYOUTS, AdamCase

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_bits.json")
ENTRIES = ("step", "clip", "ls")
ARRAYS = ("param", "exp_avg", "exp_avg_sq", "image")
assert sys.byteorder == "little"


def digest(t):
    raw = t.detach().cpu().reshape(-1).contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()[:12]


def run_case(entry, layout):
    """{"<position>:n<numel>": "<param> <exp_avg> <exp_avg_sq>[ <image>]"} after the two steps; the gradients and the gaps of
    the flat layout are checked here: nothing but the four arrays may have been written"""
    c = AdamCase(layout)
    g_before = digest(c.g.cat())
    coef = torch.tensor([0.1], device=DEV) if entry == "clip" else None
    flag = torch.zeros(1, device=DEV) if entry == "ls" else None
    skipped = torch.ones(1, device=DEV) if entry == "ls" else None
    for step in ((3, 4) if entry == "ls" else (1, 2)):
        c.step_plain(step, coef, flag, skipped)
    torch.cuda.synchronize()
    assert digest(c.g.cat()) == g_before and c.gaps_ok(), (entry, layout)
    out = {}
    for i, (p, m, v, im) in enumerate(zip(c.p.t, c.m.t, c.v.t, c.img)):
        if p.numel():
            out[f"{i:02d}:n{p.numel()}"] = " ".join(digest(x) for x in (p, m, v, im) if x is not None)
    return out


def run_all():
    """every case of this process's storage build (the image is bf16 or f16: lib.STORAGE)"""
    assert ops.BF16 == (torch.bfloat16 if L.STORAGE == "bf16" else torch.float16)
    return {f"{entry}/{layout}": run_case(entry, layout) for entry in ENTRIES for layout in LAYOUTS}
