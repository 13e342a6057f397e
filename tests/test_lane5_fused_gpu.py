"""The fused backward of the stride-1 5x5 depthwise convolutions (conv_lane.hip MODE 3 at K = 5, a 12-wave workgroup on 24-channel
tiles) against the two launches it replaces -- the data gradient with the BatchNorm0 epilogue (MODE 1) and the weight gradient
(MODE 2) -- and against fp64 torch, through the C ABI.  GPU only (`pytest -m gpu`).

Bounds are the ones tests/test_kernels_gpu.py::test_dwconv_fused_backward_equals_the_two_launches holds the 3x3 fused launch to:
dZ0 bit-identical to MODE 1, BatchNorm0-backward sums to 2e-4 of the row's scale, dW to 4e-3 of the largest tap gradient."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = torch.device("cuda:0")
BF = ops.BF16
F32 = torch.float32
K, PAD = 5, 2
GUARD = 4096                  # elements of NaN in front of and behind every 16-bit operand (a multiple of 8: 16-byte alignment)


def rnd(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def banded(t):
    """the same values in the middle of a NaN-filled allocation: whatever a launch reads beside the tensor is a NaN"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=DEV, dtype=t.dtype)
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


def bn_stats(e, c, rows, seed):
    gamma, beta = rnd(c, seed=seed, dtype=F32) * 0.2 + 1.0, rnd(c, seed=seed + 1, dtype=F32) * 0.1
    ef = e.float()
    mean, var = ef.mean(0), ef.var(0, unbiased=False)
    st = ops.BNStats()
    st.mean, st.invstd = mean.contiguous(), (var + 1e-3).rsqrt().contiguous()
    st.scale = (gamma * st.invstd).contiguous()
    st.shift = (beta - mean * st.scale).contiguous()
    st.count = float(rows)
    return st


def dw_ref64(a0, g, n, h, w, c):
    """dW[kh*K+kw, c] = sum g[o, j] * a0[o - PAD + kh, j - PAD + kw] in fp64"""
    xp = torch.zeros((n, h + 2 * PAD, w + 2 * PAD, c), dtype=torch.float64, device=DEV)
    xp[:, PAD:PAD + h, PAD:PAD + w] = a0.double().view(n, h, w, c)
    gg = g.double().view(n, h, w, c)
    return torch.stack([(gg * xp[:, kh:kh + h, kw:kw + w]).sum((0, 1, 2)) for kh in range(K) for kw in range(K)])


def two_launches(dd, e, st, wk, wflip, n, h, w, c):
    """MODE 1 + MODE 2 in their lane = column forms"""
    lib = L.load()
    old = lib.mc_dwconv_set_lane_mode(1)
    try:
        dz, part = ops.dwconv_bwd_data(dd, wk, n, h, w, c, K, 1, PAD, PAD, h, w, w_kkc_flipped=wflip, epi=(e, st))
        dw = ops.dwconv_bwd_weight(e, dd, n, h, w, c, K, 1, PAD, PAD, h, w, pro=(st.scale, st.shift))
    finally:
        lib.mc_dwconv_set_lane_mode(old)
    return dz, part, dw


def fused(dd, e, st, wflip, n, h, w, c, det, prefill):
    """one mc_dwconv_bwd_fused launch through the C ABI: the workspaces have exactly the promised rows and start as NaN, dw_out
    starts as `prefill`.  Returns dZ0, stat_partials, dw_out, dw_partials (None with the atomic ending)."""
    lib = L.load()
    a = ops._dw_fused_args(dd, wflip, n, h, w, c, K, PAD, PAD, h, w, e, st)
    dz = torch.full((n * h * w, c), float("nan"), dtype=BF, device=DEV)
    rows = lib.mc_dwconv_bwd_fused_stat_rows(C.byref(a))
    assert rows >= 1
    part = torch.full((rows, 2, c), float("nan"), dtype=F32, device=DEV)
    dw = prefill.clone()
    a.out, a.dw_out, a.stat_partials, a.stat_rows = dz.data_ptr(), dw.data_ptr(), part.data_ptr(), rows
    ws = None
    if det:
        drows = lib.mc_dwconv_bwd_fused_dw_rows(C.byref(a))
        assert drows >= 1
        ws = torch.full((drows, K * K, c), float("nan"), dtype=F32, device=DEV)
        a.dw_partials, a.dw_rows = ws.data_ptr(), drows
    L.call("mc_dwconv_bwd_fused", C.byref(a), ops._st())
    return dz, part, dw, ws


def relmax(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# n, h, w, c.  One output column per lane: a strip is 60 columns, two images share a wave where the map has at most 29 columns
# (33 staged columns per image) and there are at least two images.
CASES = [
    (1, 3, 29, 24),        # shorter than the kernel and than the 4-row block; one image: a 29-column map in a one-image wave; one tile
    (2, 4, 29, 48),        # two images per wave, exactly one block; two tiles
    (3, 5, 29, 40),        # ragged image group (3 = 2 + 1), ragged last tile (40 = 24 + 16)
    (5, 9, 29, 8),         # ragged image group, one vector of one tile; the five-row accumulator rotation wraps once
    (2, 9, 57, 24),        # 57 columns: one strip, the lanes beyond it idle
    (1, 5, 60, 40),        # exactly one strip
    (3, 4, 61, 8),         # a second strip of one column
    (1, 9, 64, 48),        # the 64- and 65-column maps: second strips of 4 and 5 columns
    (2, 3, 65, 24),
    (5, 5, 130, 40),       # a partial third strip; items end inside blocks
    (1, 70000, 9, 8),      # 128 workgroups x 547 rows: 138 blocks each -- past the 128-slot ring, whose refill they read once
]


@pytest.mark.parametrize("n,h,w,c", CASES)
def test_fused_5x5_backward_equals_the_two_launches(n, h, w, c):
    """Every demand of the 3x3 fused launch, at K = 5: dZ0 bit-identical to MODE 1; the BatchNorm0-backward sums (of the stored
    dZ0, as the kernel forms them) and dW against fp64; workspaces of exactly the promised rows, NaN before and finite after;
    dw_out accumulated into; the store-and-sum ending bit-identical between two runs and equal to the atomic ending in dZ0 and
    the statistics.  A launch on all-NaN operands runs first, so every LDS slot holds a NaN pattern when the launches under test
    start; dd and e lie between NaN guard bands."""
    e, dd = banded(rnd(n * h * w, c, seed=1)), banded(rnd(n * h * w, c, seed=2))
    wk = rnd(K * K, c, seed=3, dtype=F32)
    st = bn_stats(e, c, n * h * w, 4)
    wflip = wk.flip(0).contiguous()
    lib = L.load()
    a = ops._dw_fused_args(dd, wflip, n, h, w, c, K, PAD, PAD, h, w, e, st)
    assert lib.mc_dwconv_bwd_fused5_supported(C.byref(a)) and not lib.mc_dwconv_bwd_fused_supported(C.byref(a))
    dz_ref, _, dw_sep = two_launches(dd, e, st, wk, wflip, n, h, w, c)
    z = e.double() * st.scale.double() + st.shift.double()
    dw64 = dw_ref64(z * torch.sigmoid(z), dd, n, h, w, c)
    s64 = torch.stack([dz_ref.double().sum(0), (dz_ref.double() * (e.double() - st.mean.double()) * st.invstd.double()).sum(0)])
    pre = rnd(K * K, c, seed=9, dtype=F32)
    nan = torch.full_like(e, float("nan"))
    fused(nan, nan, st, wflip, n, h, w, c, False, pre)
    dz, part, dw, _ = fused(dd, e, st, wflip, n, h, w, c, False, pre)
    det = [fused(dd, e, st, wflip, n, h, w, c, True, pre) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(dz, dz_ref), "fused dZ0 differs from the MODE 1 launch"
    assert torch.isfinite(part).all() and torch.isfinite(dw).all()
    s = part.double().sum(0)
    fig = dict(sums=float(((s - s64).abs() / s64.abs().amax(dim=1, keepdim=True)).max()),
               dw64=relmax(dw - pre, dw64), dw_sep=relmax(dw - pre, dw_sep), dw64_det=relmax(det[0][2] - pre, dw64))
    print((n, h, w, c), fig)
    assert fig["sums"] <= 2e-4, fig
    assert fig["dw64"] <= 4e-3 and fig["dw_sep"] <= 4e-3 and fig["dw64_det"] <= 4e-3, fig
    for dz_d, part_d, dw_d, ws_d in det:
        assert torch.equal(dz_d, dz) and torch.equal(part_d, part), "the store-and-sum launch differs in dZ0 / the statistics"
        assert torch.isfinite(ws_d).all(), "a dw_partials element was not written"
    assert torch.equal(det[0][2], det[1][2]) and torch.equal(det[0][3], det[1][3]), "the store-and-sum ending is not reproducible"


def test_wrong_workspace_rows_are_refused():
    n, h, w, c = 2, 9, 57, 24
    e, dd = rnd(n * h * w, c, seed=1), rnd(n * h * w, c, seed=2)
    st = bn_stats(e, c, n * h * w, 4)
    wflip = rnd(K * K, c, seed=3, dtype=F32)
    lib = L.load()
    a = ops._dw_fused_args(dd, wflip, n, h, w, c, K, PAD, PAD, h, w, e, st)
    rows = lib.mc_dwconv_bwd_fused_stat_rows(C.byref(a))
    dz, dw = torch.empty((n * h * w, c), dtype=BF, device=DEV), torch.zeros((K * K, c), dtype=F32, device=DEV)
    part = torch.empty((rows, 2, c), dtype=F32, device=DEV)
    ws = torch.full((rows + 1, K * K, c), float("nan"), dtype=F32, device=DEV)
    a.out, a.dw_out, a.stat_partials, a.stat_rows = dz.data_ptr(), dw.data_ptr(), part.data_ptr(), rows
    a.dw_partials, a.dw_rows = ws.data_ptr(), rows + 1
    assert lib.mc_dwconv_bwd_fused(C.byref(a), ops._st()) != 0 and b"dw_partials" in lib.mc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(ws).all() and not dw.any()
    # the form whose e rows are formed from the block input exists for 3x3 only
    a.xw, a.cin = 16, 64
    assert not lib.mc_dwconv_bwd_fused5_supported(C.byref(a))


def _worker(fused_flag):
    p = subprocess.run([sys.executable, os.path.join(HERE, "_lane5_block_worker.py")], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, MC_DW_FUSED=str(fused_flag)), timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("LANE5-BLOCK-WORKER ")][-1]
    return json.loads(line[len("LANE5-BLOCK-WORKER "):])


def test_block_backward_fused_against_two_launches():
    """One MBConv block with the geometry of B5 block 21 scaled down (5x5, stride 1, 176 -> 1056 -> 176 at 2 x 24 x 29), forward +
    backward, MC_DW_FUSED=1 against =0 in fresh processes (the variable is read once per process).  Forward bit-identical; every
    gradient within the bounds of test_model_gpu.py::test_round5_fusions_same_forward_close_gradients: cosine >= 0.998 where the
    gradient is not noise-sized (> 5 % of the block's gradient scale G), else within 1e-2 G."""
    two, one = _worker(0), _worker(1)
    assert two["fused_dw5"] is False and one["fused_dw5"] is True, (two["fused_dw5"], one["fused_dw5"])
    assert one["y"] == two["y"], "forward differs"
    G = max(max(abs(v) for v in g) for g in two["grads"].values())
    worst = (1.0, "")
    for name, g in two["grads"].items():
        a_, b_ = torch.tensor(g, dtype=torch.float64), torch.tensor(one["grads"][name], dtype=torch.float64)
        if float(a_.abs().max()) > 0.05 * G:
            cos = float((a_ @ b_) / (a_.norm() * b_.norm()))
            worst = min(worst, (cos, name))
            assert cos >= 0.998, (name, cos)
        else:
            assert float((a_ - b_).abs().max()) <= 1e-2 * G, name
    print("5x5 block, fused against two launches: worst gradient cosine", worst)
