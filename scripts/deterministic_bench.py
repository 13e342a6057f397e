#!/usr/bin/env python3
"""Times the deterministic mode (ops.set_deterministic: store-and-sum endings instead of float atomics)
against the default mode, per site, in one process: HIP events after a warm-up, the two arms alternating, REPS repeats, median.

  add_ln_bwd        16384 x 768, p = 0.1
  embed_bwd         b = 64, T = 256, the real vocabulary (28996 x 768), ids ~ the tokenizer's: [CLS] ... [SEP] then [PAD]
  dw_bww_3x3        mc_dwconv_bwd_weight, 32 x 95 x 57 x 768 (B5 stage 5)
  dw_bww_5x5        mc_dwconv_bwd_weight, 32 x 48 x 29 x 1824 (B5 stage 6)
  dw_fused_3x3      mc_dwconv_bwd_fused, 32 x 95 x 57 x 768
  dw_s2_xw          mc_dwconv_bwd_data with xw + dw_out, 32 x 190 x 114, 64 -> 384 channels

The workspace bytes of each site are computed from the shapes by the library's sizing helpers.  Prints one JSON line.
The whole-step arms (default mode against the commit before inside that commit's own spread; deterministic against default on
the cfg3 step) are not part of this script yet; DESIGN.md section 9h says so.

    python scripts/deterministic_bench.py [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mammo_clip_amd import lib as L, ops  # noqa: E402

DEV = torch.device("cuda:0")


def rnd(*shape, seed=0, dtype=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV).to(ops.BF16 if dtype is None else dtype)


def ab_us(fn, reps, warmup=3):
    """median microseconds of fn() in the default and in the deterministic mode, the arms alternating"""
    us = {False: [], True: []}
    for det in (False, True):
        ops.set_deterministic(det)
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for det in (False, True):
            ops.set_deterministic(det)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us[det].append(e0.elapsed_time(e1) * 1e3)
    ops.set_deterministic(False)
    return {"default_us": round(statistics.median(us[False]), 1), "deterministic_us": round(statistics.median(us[True]), 1)}


def bn_stats(e, c, rows):
    ef = e.float()
    st = ops.BNStats()
    st.mean, var = ef.mean(0).contiguous(), ef.var(0, unbiased=False)
    st.invstd = (var + 1e-3).rsqrt().contiguous()
    st.scale, st.shift, st.count = st.invstd.clone(), (-st.mean * st.invstd).contiguous(), float(rows)
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    reps = ap.parse_args().reps
    lib = L.load()
    out = {}

    rows, h = 16384, 768
    dy, x, res = rnd(rows, h, seed=1), rnd(rows, h, seed=2), rnd(rows, h, seed=3)
    gamma = rnd(h, seed=4, dtype=torch.float32)
    mean, rstd = rnd(rows, seed=5, dtype=torch.float32), rnd(rows, seed=6, dtype=torch.float32).abs() + 0.5
    out["add_ln_bwd"] = dict(ab_us(lambda: ops.add_ln_bwd(dy, x, res, gamma, mean, rstd, 0.1, 5, 2), reps),
                             ws_bytes=lib.mc_add_ln_bwd_ws_rows(rows) * 2 * h * 4)

    b, t, vocab = 64, 256, 28996
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(1000, vocab, (b, t), generator=g)
    ln = torch.randint(8, t + 1, (b,), generator=g)
    ids[torch.arange(t)[None, :] >= ln[:, None]] = 0
    ids[:, 0] = 101
    ids, tt = ids.to(DEV), torch.zeros(b, t, dtype=torch.int64, device=DEV)
    word, pos, typ = rnd(vocab, h, seed=8, dtype=torch.float32), rnd(512, h, seed=9, dtype=torch.float32), rnd(2, h, seed=10, dtype=torch.float32)
    y, mean_e, rstd_e = ops.bert_embed_fwd(ids, tt, word, pos, typ, gamma, gamma, 1e-12, 0.1, 11, 3)
    dye = rnd(b * t, h, seed=11)
    out["embed_bwd"] = dict(ab_us(lambda: ops.bert_embed_bwd(dye, ids, tt, word, pos, typ, gamma, mean_e, rstd_e, 0.1, 11, 3), reps),
                            ws_bytes=lib.mc_bert_embed_bwd_ws_floats(b, t, h, b * t, None) * 4, pad_fraction=round(float((ids == 0).float().mean()), 3))

    def dw_bytes(fn, a):
        return getattr(lib, fn)(C.byref(a)) * a.k * a.k * a.c * 4

    for name, (n, hh, w, c, k) in {"dw_bww_3x3": (32, 95, 57, 768, 3), "dw_bww_5x5": (32, 48, 29, 1824, 5)}.items():
        xx, dd = rnd(n * hh * w, c, seed=12), rnd(n * hh * w, c, seed=13)
        a = ops._dw_args(n, hh, w, c, k, 1, k // 2, k // 2, hh, w)
        out[name] = dict(ab_us(lambda: ops.dwconv_bwd_weight(xx, dd, n, hh, w, c, k, 1, k // 2, k // 2, hh, w), reps),
                         ws_bytes=dw_bytes("mc_dwconv_bwd_weight_dw_rows", a))
        del xx, dd

    n, hh, w, c = 32, 95, 57, 768
    e, dd = rnd(n * hh * w, c, seed=14), rnd(n * hh * w, c, seed=15)
    st, wflip = bn_stats(e, c, n * hh * w), rnd(9, c, seed=16, dtype=torch.float32)
    a = ops._dw_fused_args(dd, wflip, n, hh, w, c, 3, 1, 1, hh, w, e, st)
    out["dw_fused_3x3"] = dict(ab_us(lambda: ops.dwconv_bwd_fused(dd, e, st, wflip, n, hh, w, c, 3, 1, 1, hh, w), reps),
                               ws_bytes=dw_bytes("mc_dwconv_bwd_fused_dw_rows", a))
    del e, dd

    n, hh, w, cin, c = 32, 190, 114, 64, 384
    oh, ow = (hh + 1) // 2, (w + 1) // 2
    xb, we = rnd(n * hh * w, cin, seed=17), (rnd(c, cin, seed=18).float() * cin ** -0.5).to(ops.BF16)
    dd, wk = rnd(n * oh * ow, c, seed=19), rnd(9, c, seed=20, dtype=torch.float32)
    st = bn_stats(ops.linear_fwd(xb, we), c, n * hh * w)
    a = ops._dw_args(n, hh, w, c, 3, 2, 0, 1, oh, ow)
    a.epi_x, a.xw, a.cin = 16, 16, cin
    out["dw_s2_xw"] = dict(ab_us(lambda: ops.dwconv_bwd_data(dd, wk, n, hh, w, c, 3, 2, 0, 1, oh, ow, epi=(None, st), xw=(xb, we), dw=True), reps),
                           ws_bytes=dw_bytes("mc_dwconv_bwd_data_dw_rows", a))
    print(json.dumps({"deterministic_bench": out, "storage": L.STORAGE, "reps": reps}))


if __name__ == "__main__":
    main()
