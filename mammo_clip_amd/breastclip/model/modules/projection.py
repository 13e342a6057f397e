"""Projection heads [ref: model/modules/projection.py:4-29].  The linear head (the one every pre-training config
uses) runs as an fp32 HIP GEMM, the MLP head as fp32 HIP GEMMs plus the row / pointwise kernels of csrc/head.hip; the L2
normalisation lives in model/clip.py like in the reference."""
import torch
from torch import nn

from .... import ops


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        m, k = x.shape
        n = w.shape[0]
        y = torch.empty((m, n), dtype=torch.float32, device=x.device)
        ops.sgemm(x, k, 1, w, 1, k, y, n, m, n, k, bias=b)          # y = x @ w.T + b
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        m, k = x.shape
        n = w.shape[0]
        dx = torch.empty_like(x)
        ops.sgemm(dy, n, 1, w, k, 1, dx, k, m, k, n)                 # dx = dy @ w
        dw = torch.empty_like(w)
        ops.sgemm(dy, 1, n, x, k, 1, dw, k, n, k, m)                 # dw = dy.T @ x
        ones = torch.ones((1, m), dtype=torch.float32, device=x.device)
        db = torch.empty((1, n), dtype=torch.float32, device=x.device)
        ops.sgemm(ones, m, 1, dy, n, 1, db, n, 1, n, m)              # db = sum_rows dy
        return dx, dw, db.view(n)


class LinearProjectionHead(nn.Module):
    def __init__(self, embedding_dim, projection_dim):
        super().__init__()
        self.projection = nn.Linear(embedding_dim, projection_dim)   # parameter container

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("mammo_clip_amd.LinearProjectionHead runs only on a HIP device (no CPU fallback)")
        return _LinearFn.apply(x.float(), self.projection.weight, self.projection.bias)


class _MLPHeadFn(torch.autograd.Function):
    """p = x W1^T + b1;  g = GELU(p);  f = g W2^T + b2;  y = LayerNorm(dropout(f) + p) * gamma + beta, all fp32.
    Saved: x, p, xhat, rstd (O(m n)); g is recomputed for the fc weight gradient and the dropout mask is regenerated from
    (seed, stream_id).  Launches per call: forward 4 (two mc_sgemm, GELU, the row kernel), backward 12 with every gradient
    wanted (row kernel + 3 ordered sums, GELU, 5 mc_sgemm + the ones fill of the bias sum, GELU backward); a split-K
    mc_sgemm adds its finish launch."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, eps, p, seed, stream_id):
        x = x.contiguous()
        m, k = x.shape
        n = w1.shape[0]
        pr = torch.empty((m, n), dtype=torch.float32, device=x.device)
        ops.sgemm(x, k, 1, w1, 1, k, pr, n, m, n, k, bias=b1)        # p = x @ w1.T + b1
        g = ops.gelu_f32_fwd(pr)
        f = torch.empty_like(pr)
        ops.sgemm(g, n, 1, w2, 1, n, f, n, m, n, n, bias=b2)         # f = g @ w2.T + b2
        y, xhat, rstd = ops.mlp_head_ln_fwd(f, pr, gamma, beta, eps, p, seed, stream_id)
        ctx.save_for_backward(x, pr, xhat, rstd, w1, w2, gamma)
        ctx.drop = (p, seed, stream_id)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pr, xhat, rstd, w1, w2, gamma = ctx.saved_tensors
        need = ctx.needs_input_grad
        m, k = x.shape
        n = w1.shape[0]
        df, dz, dgamma, dbeta, db2 = ops.mlp_head_ln_bwd(dy.contiguous(), xhat, rstd, gamma, *ctx.drop)
        dx = dw1 = db1 = dw2 = None
        if need[3]:
            g = ops.gelu_f32_fwd(pr)
            dw2 = torch.empty_like(w2)
            ops.sgemm(df, 1, n, g, n, 1, dw2, n, n, n, m)            # dw2 = df.T @ g
        if need[0] or need[1] or need[2]:
            dg = torch.empty_like(df)
            ops.sgemm(df, n, 1, w2, n, 1, dg, n, m, n, n)            # dg = df @ w2
            dp = ops.gelu_f32_bwd_add(dg, pr, dz)                    # fc branch + residual branch
            if need[0]:
                dx = torch.empty_like(x)
                ops.sgemm(dp, n, 1, w1, k, 1, dx, k, m, k, n)        # dx = dp @ w1
            if need[1]:
                dw1 = torch.empty_like(w1)
                ops.sgemm(dp, 1, n, x, k, 1, dw1, k, n, k, m)        # dw1 = dp.T @ x
            if need[2]:
                ones = torch.ones((1, m), dtype=torch.float32, device=x.device)
                db1 = torch.empty((1, n), dtype=torch.float32, device=x.device)
                ops.sgemm(ones, m, 1, dp, n, 1, db1, n, 1, n, m)     # db1 = sum_rows dp
                db1 = db1.view(n)
        return (dx, dw1, db1, dw2, db2 if need[4] else None, dgamma if need[5] else None, dbeta if need[6] else None,
                None, None, None, None)


class MLPProjectionHead(nn.Module):
    """[ref: model/modules/projection.py:4-20]  Linear -> GELU -> Linear -> dropout -> + the first Linear's output -> LayerNorm,
    as one autograd function over fp32 HIP kernels (csrc/head.hip).  ``projection``, ``fc``,
    ``layer_norm`` and ``dropout`` are parameter / setting containers with the reference's names and default initialisation.

    Dropout masks are counter-based: ``forward(x, seed, stream_id)`` draws the mask of (seed, stream_id); BreastClip derives the
    seed from the call counter of the encoder that produced ``x`` so that a re-forward after rewinding the encoders' counters
    (engine micro-batching) reproduces it.  Called without a seed the head counts its own calls."""
    rng_seed = 0x4EAD
    max_projection_dim = 2048          # = mc_mlp_head_max_n()

    def __init__(self, embedding_dim, projection_dim, dropout):
        super().__init__()
        # (pure Python on purpose: constructing a head must not need the kernel library; tests pin it to mc_mlp_head_supported)
        if projection_dim % 8 != 0 or not 8 <= projection_dim <= self.max_projection_dim:
            raise ValueError(f"MLPProjectionHead: proj_dim must be a multiple of 8 in [8, {self.max_projection_dim}] "
                             f"(the row kernels hold a row in registers), got {projection_dim}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"MLPProjectionHead: dropout must be in [0, 1), got {dropout}")
        self.projection = nn.Linear(embedding_dim, projection_dim)
        self.fc = nn.Linear(projection_dim, projection_dim)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(projection_dim)
        self._calls = 0
        self.last_seed = None          # (seed, stream_id) of the latest train-mode call with dropout, for inspection

    def forward(self, x, seed=None, stream_id=0):
        if not x.is_cuda:
            raise RuntimeError("mammo_clip_amd.MLPProjectionHead runs only on a HIP device (no CPU fallback)")
        p = float(self.dropout.p) if self.training else 0.0
        if p > 0.0:
            if seed is None:
                self._calls += 1
                seed = self._calls
            seed = self.rng_seed * 1000003 + int(seed)
            self.last_seed = (seed, int(stream_id))
        else:
            seed = 0
        ln = self.layer_norm
        return _MLPHeadFn.apply(x.float(), self.projection.weight, self.projection.bias, self.fc.weight, self.fc.bias,
                                ln.weight, ln.bias, float(ln.eps), p, seed, int(stream_id))
