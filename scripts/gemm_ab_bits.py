#!/usr/bin/env python3
"""Bit-for-bit A/B of the tiled GEMM family (gemm.hip, gemm256.hip, gemm256_tn.hip): runs the seeded GEMM cases of
tests/test_kernels_gpu.py and prints one SHA-256 per case and route over the output tensor (and the statistics partials where
the case asks for them).  Every GEMM here sums in a fixed order, so two builds of the library must print the same digests:
    bash scripts/ab_libs.sh "parent base" python scripts/gemm_ab_bits.py     (GPU box; ab/parent.so from scripts/ab_variant.sh)
No accumulating (c_atomic) call is included.  Routes: default = the library's own rule; MC_GEMM_256 / MC_GEMM_256TN = 2 force the
256 x 256 kernels wherever the layout allows, MC_GEMM_256TN = 0 forces the 128-row family for TN problems."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mammo_clip_amd  # noqa: F401,E402
from mammo_clip_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16


def rnd(*shape, seed=0, scale=1.0, dtype=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype or BF)


class route:
    """environment switch for the launches inside; route(None, None) = the default rule"""

    def __init__(self, var, val):
        self.var, self.val = var, val

    def __enter__(self):
        if self.var:
            self.old = os.environ.get(self.var)
            os.environ[self.var] = self.val

    def __exit__(self, *a):
        if self.var:
            if self.old is None:
                os.environ.pop(self.var, None)
            else:
                os.environ[self.var] = self.old

    def __str__(self):
        return f"{self.var}={self.val}" if self.var else "default"


DEFAULT, F256, FTN, NOTN = route(None, None), route("MC_GEMM_256", "2"), route("MC_GEMM_256TN", "2"), route("MC_GEMM_256TN", "0")


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        c = t.detach().contiguous().cpu()
        h.update(str((tuple(c.shape), str(c.dtype))).encode())
        h.update(c.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def emit(case, r, *tensors):
    torch.cuda.synchronize()
    print(f"{case:58s} {str(r):18s} {digest(*tensors)}", flush=True)


def nt(M, N, K, routes, name):
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    for r in routes:
        with r:
            emit(f"{name}[{M}-{N}-{K}]", r, ops.linear_fwd(x, w))


def dgrad_nn(M, N, K):
    dy, w, res = rnd(M, N, seed=8), rnd(N, K, seed=9, scale=N ** -0.5), rnd(M, K, seed=10)
    emit(f"gemm_dgrad_nn[{M}-{N}-{K}]", DEFAULT, ops.linear_dgrad(dy, w, residual=res))


def wgrad_tn(M, N, K, routes, name):
    dy, x = rnd(M, N, seed=11), rnd(M, K, seed=12)
    for r in routes:
        with r:
            emit(f"{name}[{M}-{N}-{K}]", r, ops.linear_wgrad(dy, x))


def grouped_gate(n_img, hw, N, K):
    M = n_img * hw
    x, dy = rnd(M, K, seed=101), rnd(M, N, seed=104)
    gate = torch.sigmoid(rnd(n_img, K, seed=103, dtype=torch.float32))
    for r in (DEFAULT, FTN):
        with r:
            emit(f"gemm256_tn_grouped_gate[{n_img}-{hw}-{N}-{K}]", r, ops.linear_wgrad(dy, x, pro=(None, None, gate, hw)))


def bias_residual_stats_batched_strided():
    M, N, K = 3000, 1000, 712
    x, w = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=K ** -0.5)
    bias, res = rnd(N, seed=5, dtype=torch.float32), rnd(M, N, seed=6)
    nb, hw, N2, K2 = 5, 700, 304, 1824
    xb, wb = rnd(nb * hw, K2, seed=7), rnd(nb, N2, K2, seed=8, scale=K2 ** -0.5)
    H = 768
    xs, ws = rnd(2048, 3 * H, seed=9), rnd(H, H, seed=10, scale=H ** -0.5)
    for r in (DEFAULT, F256):
        with r:
            emit("bias+residual", r, ops.linear_fwd(x, w, bias=bias, residual=res))
            y3, part = ops.linear_fwd(x, w, stats=True)
            emit("stats", r, y3, part)
            yb = torch.empty(nb * hw, N2, device=DEV, dtype=BF)
            pb = ops.gemm(xb, wb, yb, hw, N2, K2, K2, K2, N2, batch=nb, sA=(hw * K2, 0), sB=(N2 * K2, 0), sC=(hw * N2, 0),
                          alpha=0.5, stats=True)
            emit("batched+alpha+stats", r, yb, pb)
            out = torch.zeros(2048, 3 * H, device=DEV, dtype=BF)
            ops.gemm(xs[:, H:], ws, out[:, 2 * H:], 2048, H, H, 3 * H, H, 3 * H)
            emit("strided", r, out)
    # the 128-row family's bias / gelu-input / residual / stats case
    M, N, K = 700, 3072, 768
    x, w = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=K ** -0.5)
    bias = rnd(N, seed=5, dtype=torch.float32)
    y = ops.linear_fwd(x, w, bias=bias)
    emit("gemm_bias", DEFAULT, y)
    res, w2 = rnd(M, 768, seed=6), rnd(768, N, seed=7, scale=N ** -0.5)
    emit("gemm_bias+residual", DEFAULT, ops.linear_fwd(y, w2, bias=bias[:768].contiguous(), residual=res))
    emit("gemm_stats", DEFAULT, *ops.linear_fwd(x, w, stats=True))


def empty_split(M, N):
    K, splits = 576, 4
    a, b = rnd(K, M, seed=21), rnd(K, N, seed=22)
    for r in (DEFAULT, NOTN, FTN):
        ws = torch.full((splits, M, N), float("nan"), device=DEV, dtype=torch.float32)
        c = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32)
        with r:
            ops.gemm(a, b, c, M, N, K, M, N, N, a_kmajor=1, b_kmajor=1, c_f32=1, splits=splits, splitk_ws=ws)
        emit(f"gemm_tn_empty_split[{M}-{N}]", r, c, ws)


if __name__ == "__main__":
    for s in [(300, 144, 24), (1000, 24, 144), (257, 40, 240), (129, 1408, 352), (512, 768, 768), (77, 16, 16), (4096, 304, 1824),
              (130, 64, 48)]:
        nt(*s, (DEFAULT,), "gemm_nt")
    for s in [(300, 24, 144), (1000, 240, 40), (513, 352, 1408), (64, 768, 3072)]:
        dgrad_nn(*s)
    for s in [(5000, 144, 24), (3000, 24, 144), (70000, 240, 40), (1392, 1824, 304), (999, 48, 32)]:
        wgrad_tn(*s, (DEFAULT, NOTN), "gemm_wgrad_tn")
    for s in [(256, 256, 64), (512, 256, 128), (300, 144, 24), (257, 40, 240), (4096, 304, 1824), (5000, 1824, 304),
              (1392 * 3, 512, 3072), (8192, 2304, 768), (777, 776, 1000), (66000, 176, 1056), (130, 64, 48), (20000, 3072, 512)]:
        nt(*s, (DEFAULT, F256), "gemm256_nt")
    for s in [(4096, 304, 1824), (44544, 1824, 304), (5000, 176, 1056), (16384, 768, 3072), (3000, 264, 40), (700, 256, 256),
              (64, 8, 8)]:
        wgrad_tn(*s, (DEFAULT, FTN), "gemm256_tn_wgrad")
    for s in [(4, 1392, 304, 1824), (3, 5415, 176, 1056), (5, 700, 512, 3072)]:
        grouped_gate(*s)
    bias_residual_stats_batched_strided()
    for s in [(136, 264), (40, 24)]:
        empty_split(*s)
