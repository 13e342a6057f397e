"""The fused depthwise backward (conv_lane.hip MODE 3 / MODE 5) after the block body became straight-line code: ONE sigmoid per
element feeds both a0 = silu(bn0(e)) of the weight gradient and silu'(bn0(e)) of dZ0, and the wave-uniform row conditions
(rows beyond the item, rows that do not count for the statistics) are folded into the column masks instead of branches.
GPU only (`pytest -m gpu`).  Every bound below is the one tests/test_kernels_gpu.py already uses for the same quantity."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16
GUARD = 4096                  # elements of NaN in front of and behind every 16-bit operand (a multiple of 8: 16-byte alignment)


@pytest.fixture(autouse=True)
def _kernel_switches_on():
    old = ops.XDW, ops.EFREE
    ops.XDW, ops.EFREE = 1, 1
    yield
    ops.XDW, ops.EFREE = old


def rnd(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def banded(t):
    """the same values in the middle of a NaN-filled allocation: whatever a launch reads in front of or behind the tensor (a row
    above the first image, below the last one) is a NaN"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=DEV, dtype=t.dtype)
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


def bn_stats(e, c, n, h, w, seed):
    gamma, beta = rnd(c, seed=seed, dtype=torch.float32) * 0.2 + 1.0, rnd(c, seed=seed + 1, dtype=torch.float32) * 0.1
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(n * h * w)
    return st


def mode1(dd, e, st, wk, wflip, n, h, w, c):
    """the data-gradient launch with the BatchNorm-backward epilogue in its lane = column form (conv_lane.hip MODE 1)"""
    Lh = L.load()
    old = Lh.mc_dwconv_set_lane_mode(1)
    try:
        return ops.dwconv_bwd_data(dd, wk, n, h, w, c, 3, 1, 1, 1, h, w, w_kkc_flipped=wflip, epi=(e, st))
    finally:
        Lh.mc_dwconv_set_lane_mode(old)


def partials_close(part_ref, part, tol):
    s0, s1 = part_ref.double().sum(0), part.double().sum(0)
    scale = s0.abs().amax(dim=1, keepdim=True)
    return float(((s0 - s1).abs() / scale).max()) <= tol


# n, h, w, c
CASES = [
    (2, 70, 300, 48),      # several strips per row, ragged channel tile, items that end inside a block
    (3, 33, 59, 24),       # h = 33: the last block of every image has ONE e row (rows beyond the item: erhi < ORB)
    (33, 48, 29, 64),      # image groups (two images per wave), 33 images: the last group is ragged
    (9, 7, 9, 24),         # tiny maps, ragged last group, rows beyond the item in every block
    (2, 40, 33, 240),
    (70, 600, 40, 32),     # > 128 blocks per workgroup: the descriptor ring is refilled (now from one call site per loop trip)
]


@pytest.mark.parametrize("n,h,w,c", CASES)
def test_fused_backward_one_sigmoid_equals_the_epilogue_launch(n, h, w, c):
    """MODE 3 against the two launches it replaces.  dZ0 must equal the MODE 1 launch BIT FOR BIT (silu' is now taken from the
    sigmoid evaluated when the row entered the window -- the same expressions as silu2_f / silu_grad2_f); dW and the
    BatchNorm0-backward partials must be finite and within the bounds of test_dwconv_fused_backward_equals_the_two_launches
    (partials 2e-4 of the column's scale, dW 4e-3 of the largest tap gradient against the separate weight-gradient launch).

    Before the launches under test, one launch runs on operands that are NaN everywhere: dd fills the input tiles, e the e tile
    and dZ0 = NaN the output tile, so every LDS slot a launch can reach holds a NaN pattern when the next launch starts on that
    CU.  e and dd sit between NaN guard bands in memory.  Non-finite e in rows / columns that do not exist cannot be placed
    through the API otherwise: the operands are dense NHWC tensors, rows beyond an item and columns beyond the map have no
    address of their own (the kernel clamps such loads to the tensor's first pixel and masks the value)."""
    k, pad = 3, 1
    e, dd = banded(rnd(n * h * w, c, seed=1)), banded(rnd(n * h * w, c, seed=2))
    wk = rnd(k * k, c, seed=3, dtype=torch.float32)
    st = bn_stats(e, c, n, h, w, 4)
    wflip = wk.flip(0).contiguous()
    assert ops.dwconv_bwd_fused_ok(n, h, w, c, k, 1, pad, pad, h, w, force=True)
    dz_ref, part_ref = mode1(dd, e, st, wk, wflip, n, h, w, c)
    dw_sep = ops.dwconv_bwd_weight(e, dd, n, h, w, c, k, 1, pad, pad, h, w, pro=(st.scale, st.shift))
    nan = torch.full_like(e, float("nan"))
    ops.dwconv_bwd_fused(nan, nan, st, wflip, n, h, w, c, k, pad, pad, h, w)
    for _ in range(2):
        dz, part, dw = ops.dwconv_bwd_fused(dd, e, st, wflip, n, h, w, c, k, pad, pad, h, w)
    torch.cuda.synchronize()
    assert torch.equal(dz, dz_ref), "fused dZ0 differs from the MODE 1 launch"
    assert torch.isfinite(part).all() and torch.isfinite(dw).all()
    assert partials_close(part_ref, part, 2e-4), "BatchNorm-backward partials"
    assert float((dw - dw_sep).abs().max()) <= 4e-3 * float(dw_sep.abs().max()), "dW vs the separate weight-gradient launch"


# n, h, w, cin, c
XE_CASES = [(2, 70, 300, 40, 240), (3, 33, 59, 24, 144), (5, 95, 57, 64, 72), (33, 48, 29, 16, 96), (9, 7, 9, 8, 24)]


@pytest.mark.parametrize("n,h,w,cin,c", XE_CASES)
def test_fused_backward_e_from_block_input_one_sigmoid(n, h, w, cin, c):
    """MODE 5 (e rows formed from the block input by the MFMA staging).  The expand weight is a 0/1 selection matrix, so the
    staged e IS x[:, sel] exactly and dZ0 must equal the MODE 1 launch on e = x[:, sel] BIT FOR BIT; the partials and dW are
    held to the bounds of test_dwconv_fused_backward_with_e_rows_formed_from_the_block_input against the launch that reads e
    (2e-3 of the column's scale, 2e-3 of the largest tap gradient).  NaN-poisoned LDS and guard bands as in the test above."""
    k, pad = 3, 1
    x = banded(rnd(n * h * w, cin, seed=71))
    sel = torch.arange(c, device=DEV) * 7 % cin                 # asymmetric: expanded channel i reads input channel 7 i mod cin
    we = torch.zeros(c, cin, device=DEV)
    we[torch.arange(c, device=DEV), sel] = 1.0
    we = we.to(BF)
    e = banded(x[:, sel].contiguous())
    dd = banded(rnd(n * h * w, c, seed=73))
    wk = rnd(k * k, c, seed=74, dtype=torch.float32)
    st = bn_stats(e, c, n, h, w, 75)
    wflip = wk.flip(0).contiguous()
    assert ops.dwconv_bwd_fused_ok(n, h, w, c, k, 1, pad, pad, h, w, force=True, cin=cin)
    dz_ref, _ = mode1(dd, e, st, wk, wflip, n, h, w, c)
    _, part_ref, dw_ref = ops.dwconv_bwd_fused(dd, e, st, wflip, n, h, w, c, k, pad, pad, h, w)
    nan_x, nan_d = torch.full_like(x, float("nan")), torch.full_like(dd, float("nan"))
    ops.dwconv_bwd_fused(nan_d, None, st, wflip, n, h, w, c, k, pad, pad, h, w, xw=(nan_x, we))
    for _ in range(2):
        dz, part, dw = ops.dwconv_bwd_fused(dd, None, st, wflip, n, h, w, c, k, pad, pad, h, w, xw=(x, we))
    torch.cuda.synchronize()
    assert torch.equal(dz, dz_ref), "dZ0 (e rows from x) differs from the MODE 1 launch"
    assert torch.isfinite(part).all() and torch.isfinite(dw).all()
    assert partials_close(part_ref, part, 2e-3), "BatchNorm-backward partials"
    assert float((dw - dw_ref).abs().max()) <= 2e-3 * float(dw_ref.abs().max()), "dW"
