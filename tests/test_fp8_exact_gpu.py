"""The fp8 path of config #5 on operands for which every result is EXACT: the e4m3 quantiser and the amax kernels of
csrc/fp8.hip, the FP8 instantiations of gemm8p_kernel (csrc/gemm256.hip), ops.linear_fwd_fp8 end to end and
mc_gate_weights_bf16.  GPU only (`pytest -m gpu`).  There is no tolerance in this file: every comparison is torch.equal or a
bit pattern.

Quantiser.  Its domain is 65 536 inputs, so one launch covers it: all bit patterns of the storage type in a seeded permuted
order, under six caller-supplied amax values that are NOT the tensor's own (tests/_fp8_ref.py: thousands of inputs saturate,
thousands land in the e4m3 subnormal range, the rounding ties are counted in tests/test_fp8_exact.py).  The reference is the
first-principles table search of _fp8_ref.quant_ref on the CPU.  amax 0, a NaN amax, an amax so small that 448 / amax
overflows fp32, the amax_next output, the running maximum of mc_amax_bf16 at and one vector past the grid cap, and the
argument checks are pinned one by one.

GEMM.  The method of tests/test_gemm_exact_gpu.py, whose helpers are imported: operands are e4m3 bytes of +-1 (0x38 / 0xb8),
every product is +-1 and every partial sum an integer, so fp32 accumulation is exact in any order and the reference is an fp64
matmul.  fp8 geometry: K tiles of 128 elements, 16-element chunks, each 16-byte fragment split into two 8-byte MFMA operands;
K, lda, ldb % 16 == 0, so rows are padded by 16 bytes of 7.0 (0x4e): a read past K that reaches the accumulators moves an
output by a multiple of 7.  The output goes into a NaN-pattern guard with ldc > N.  Each case is launched twice on fresh
buffers, once under MC_GEMM_256=2 and once under MC_GEMM_256=0: mc_gemm_tile_config must say 256 both times, because the fp8
operand path exists only in that kernel.  (The bf16 path table uses K = 72 and 136; fp8 needs K % 16 == 0, so the rows here use
80 -- one ragged K tile of five chunks -- and 144 -- a full tile plus one chunk.)
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402

import _fp8_ref as R  # noqa: E402
from test_gemm_exact_gpu import (BF, DEV, F64, GATES, Guard, _id, check_rows_written, exact16, exact_stats, guard2d,  # noqa: E402
                                 nan_rows, pick, pm1, routes, store16)

F32 = torch.float32
ONE, SEVEN = 0x38, 0x4e                 # e4m3 codes of 1.0 and 7.0 (-1.0 = 0xb8)
SENT = 0xa5                             # sentinel byte around a quantised tensor
GRID_CAP = 2048 * 256 * 8               # elements one pass of the 2048-workgroup grid covers


def scalar(v):
    return torch.tensor([v], dtype=F32, device=DEV)


def bits32(t):
    return t.detach().to("cpu").contiguous().view(torch.int32)


def bits_of(v):
    return torch.tensor([v], dtype=F32).view(torch.int32)


_PATTERNS = {}


def patterns():
    """all 65 536 values of the storage type, seeded permuted order: (device tensor, the same on the CPU)"""
    if BF not in _PATTERNS:
        x = R.all_patterns(BF, seed=20)
        _PATTERNS[BF] = (x.to(DEV), x)
    return _PATTERNS[BF]


def quant_guarded(x, amax, scale_out=None, amax_next=None):
    """mc_quant_fp8_bf16 through the ABI into a byte buffer with 64 sentinel bytes on either side -> codes; the sentinels
    must come back bit-identical"""
    n = x.numel()
    buf = torch.full((64 + n + 64,), SENT, dtype=torch.uint8, device=DEV)
    L.call("mc_quant_fp8_bf16", x.data_ptr(), n, amax.data_ptr(), buf.data_ptr() + 64, ops._p(scale_out), ops._p(amax_next), ops._st())
    assert bool((buf[:64] == SENT).all()) and bool((buf[64 + n:] == SENT).all()), "a byte outside the quantised tensor changed"
    return buf[64:64 + n].clone()


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("amax", R.AMAXES, ids=lambda a: f"amax_{a:g}")
def test_quantiser_every_input_under_a_foreign_amax(amax):
    """codes == quant_ref byte for byte on every non-NaN input, a NaN code on every NaN input, scale_out == amax / 448 on bits"""
    x, x_cpu = patterns()
    a = scalar(amax)
    q, s = ops.quant_fp8(x, a)
    ref = R.quant_ref(x_cpu, torch.tensor(amax, dtype=F32))
    q_cpu, nan = q.cpu(), torch.isnan(x_cpu)
    bad = (q_cpu != ref) & ~nan
    assert not bool(bad.any()), (f"{int(bad.sum())} codes differ; first: x bits {int(x_cpu.view(torch.int16)[bad][0]) & 0xffff:#06x} "
                                 f"got {int(q_cpu[bad][0]):#04x} want {int(ref[bad][0]):#04x}")
    assert bool((q_cpu[nan] % 128 == R.NAN_CODE).all()), "a NaN input was quantised to a finite code"
    assert torch.equal(bits32(s), bits32(torch.tensor([amax], dtype=F32) / 448.0)), "scale_out is not amax / 448 in fp32"
    # the same launch through the ABI: guarded output, scale_out = None and amax_next = None accepted
    assert torch.equal(quant_guarded(x, a), q)
    nxt, s2 = torch.zeros(1, dtype=F32, device=DEV), torch.full((1,), -1.0, dtype=F32, device=DEV)
    assert torch.equal(quant_guarded(x, a, scale_out=s2, amax_next=nxt), q) and torch.equal(bits32(s2), bits32(s))
    assert bool(torch.isnan(nxt).all()), "amax_next of a tensor that holds NaN must be NaN"


def test_quantiser_amax_zero_and_nan():
    """amax 0: scale 1 and scale_out 1 (the codes are the plain rounding of x); a NaN amax: all 65 536 codes NaN"""
    x, x_cpu = patterns()
    q, s = ops.quant_fp8(x, scalar(0.0))
    nan = torch.isnan(x_cpu)
    ref = R.rne_code(x_cpu.float().clamp(-R.MAX, R.MAX))
    assert torch.equal(q.cpu()[~nan], ref[~nan]) and torch.equal(ref, R.quant_ref(x_cpu, torch.tensor(0.0)))
    assert bool((q.cpu()[nan] % 128 == R.NAN_CODE).all())
    assert torch.equal(bits32(s), bits_of(1.0))
    qn = quant_guarded(x, scalar(float("nan")))
    assert bool((qn % 128 == R.NAN_CODE).all()), f"{int((qn % 128 != R.NAN_CODE).sum())} finite codes under a NaN amax"


@pytest.mark.skipif(BF != torch.bfloat16, reason="the smallest f16 value (2^-24) cannot reach an amax whose scale overflows")
def test_quantiser_scale_stays_finite_for_a_tiny_amax():
    """amax = 2^-125: 448 / amax overflows fp32.  A finite input under a finite positive amax never gives a NaN code: +-0 stay
    0x00 / 0x80, +-amax give +-448 (0x7e / 0xfe), +-amax / 2 give +-224 (0x76 / 0xf6)"""
    amax = 2.0 ** -125
    vals = torch.tensor([0.0, -0.0, 2.0 ** -126, -2.0 ** -126, amax, -amax], dtype=torch.float32)
    want = torch.tensor([0x00, 0x80, 0x76, 0xf6, 0x7e, 0xfe], dtype=torch.uint8)
    idx = torch.randint(0, 6, (2048 * 8 + 8,), generator=torch.Generator(device="cpu").manual_seed(3))
    x_cpu = vals[idx].to(BF)
    assert torch.equal(x_cpu.float(), vals[idx])
    a = scalar(amax)
    assert float(torch.tensor(448.0) / a.cpu()) == float("inf")
    q = quant_guarded(x_cpu.to(DEV), a).cpu()
    assert not bool((q % 128 == R.NAN_CODE).any()), f"{int((q % 128 == R.NAN_CODE).sum())} NaN codes from finite inputs"
    assert torch.equal(q, want[idx]) and torch.equal(q, R.quant_ref(x_cpu, a.cpu()[0]))
    # every input at that amax (16-bit denormals aside: they are left to the no-NaN rule alone)
    x, xc = patterns()
    qa = quant_guarded(x, a).cpu()
    nan, den = torch.isnan(xc), (xc.view(torch.int16) & 0x7f80) == 0
    assert not bool((qa[~nan] % 128 == R.NAN_CODE).any())
    keep = ~nan & ~den
    assert torch.equal(qa[keep], R.quant_ref(xc, a.cpu()[0])[keep])


# ------------------------------------------------------------------------------------------------ amax
def _amax_both(x, y_amax_in, prefill=0.0):
    """the running maximum through both entry points, from a result cell prefilled with `prefill` -> (bits, bits)"""
    out = ops.amax_bf16(x, out=scalar(prefill))
    nxt = scalar(prefill)
    ops.quant_fp8(x, y_amax_in, amax_next=nxt)
    return bits32(out), bits32(nxt)


@pytest.mark.parametrize("n", [8, 2048, GRID_CAP, GRID_CAP + 8], ids=["one_vector", "one_workgroup", "grid_cap", "grid_cap_plus_one_vector"])
def test_amax_finds_one_planted_value(n):
    """zeros with one +-value at the first element, the last element, the first element of the last vector: the result is the
    planted magnitude on bits; a larger prefilled cell survives, a smaller one is replaced; zeros and -0.0 give +0; one NaN
    gives NaN -- for mc_amax_bf16 and for the amax_next output of the quantiser"""
    x = torch.zeros(n, dtype=BF, device=DEV)
    one = scalar(1.0)
    for b in _amax_both(x, one):
        assert torch.equal(b, bits_of(0.0)), "zeros must give 0"
    x.fill_(-0.0)
    assert bool(torch.signbit(x.float()).all())
    for b in _amax_both(x, one):
        assert torch.equal(b, bits_of(0.0)), "-0.0 must give +0"
    x.zero_()
    for pos, mag in zip(sorted({0, n - 1, n - 8}), (3.0, 0.8125, 2.0 ** -20)):
        for sign in (1.0, -1.0):
            x[pos] = sign * mag
            for b in _amax_both(x, one):
                assert torch.equal(b, bits_of(mag)), (n, pos, sign)
            for b in _amax_both(x, one, prefill=1000.0):
                assert torch.equal(b, bits_of(1000.0)), "a larger running maximum must survive"
            for b in _amax_both(x, one, prefill=mag / 2):
                assert torch.equal(b, bits_of(mag)), "a smaller running maximum must be replaced"
            x[pos] = 0.0
        x[pos] = float("nan")
        out, nxt = ops.amax_bf16(x), torch.zeros(1, dtype=F32, device=DEV)
        ops.quant_fp8(x, one, amax_next=nxt)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(nxt).all()), (n, pos, "a planted NaN must make the result NaN")
        x[pos] = 0.0


def test_amax_next_equals_amax_of_the_same_tensor():
    g = torch.Generator(device="cpu").manual_seed(9)
    x = (torch.randn(100_008, generator=g) * 3.0).to(BF).to(DEV)
    nxt = torch.zeros(1, dtype=F32, device=DEV)
    ops.quant_fp8(x, scalar(2.0), amax_next=nxt)
    out = ops.amax_bf16(x)
    assert torch.equal(bits32(out), bits32(nxt)) and torch.equal(bits32(out), bits32(x.float().abs().max().reshape(1)))


def test_fp8_prep_rejects_misaligned_pointers_and_ragged_sizes():
    """an error code, not a launch: the result cell, the scale and the guarded output stay as they were"""
    lib = L.load()
    x = torch.ones(64, dtype=BF, device=DEV)
    cell, a, s = scalar(-5.0), scalar(1.0), scalar(-7.0)
    y = torch.full((128,), SENT, dtype=torch.uint8, device=DEV)
    px, py, st = x.data_ptr(), y.data_ptr() + 32, ops._st()
    assert px % 16 == 0 and py % 8 == 0
    assert lib.mc_amax_bf16(px + 2, 8, cell.data_ptr(), st) != 0 and b"amax_bf16" in lib.mc_last_error()
    assert lib.mc_amax_bf16(px + 8, 8, cell.data_ptr(), st) != 0
    assert lib.mc_amax_bf16(px, 12, cell.data_ptr(), st) != 0
    assert lib.mc_amax_bf16(px, 0, cell.data_ptr(), st) != 0
    assert lib.mc_amax_bf16(px, 8, None, st) != 0
    for bad in ((px + 2, 8, py), (px + 8, 8, py), (px, 12, py), (px, 8, py + 4), (px, 8, py + 1), (px, 0, py)):
        assert lib.mc_quant_fp8_bf16(bad[0], bad[1], a.data_ptr(), bad[2], s.data_ptr(), cell.data_ptr(), st) != 0, bad
        assert b"quant_fp8_bf16" in lib.mc_last_error()
    assert lib.mc_quant_fp8_bf16(px, 8, None, py, s.data_ptr(), cell.data_ptr(), st) != 0
    torch.cuda.synchronize()
    assert float(cell) == -5.0 and float(s) == -7.0 and bool((y == SENT).all())


# ------------------------------------------------------------------------------------------------ fp8 tile GEMM
def store8(mats, extra=1):
    """[nb, R, C] fp64 of e4m3 values -> their codes in uint8 [nb, R + extra, C + 16]; the padding holds 7.0 (0x4e)"""
    codes = R.rne_code(mats)
    assert torch.equal(R.decode(codes), mats), "operand: not an e4m3 value"
    nb, r, c = mats.shape
    t = torch.full((nb, r + extra, c + 16), SEVEN, device=DEV, dtype=torch.uint8)
    t[:, :r, :c] = codes
    return t


def block_sums(ref):
    """[nb, M, N] fp64 -> [nb * ceil(M / 256), 2, N]: the column sums and sums of squares of every 256-row block"""
    nb, M, N = ref.shape
    out = []
    for z in range(nb):
        for r0 in range(0, M, 256):
            yb = ref[z, r0:r0 + 256]
            out.append(torch.stack([yb.sum(0), (yb * yb).sum(0)]))
    return torch.stack(out)


def fp8_args(M, N, K, lda, ldb, a_ptr, b_ptr):
    a = L.GemmArgs()
    a.A, a.B, a.M, a.N, a.K, a.lda, a.ldb = a_ptr, b_ptr, M, N, K, lda, ldb
    a.batch, a.nb2, a.splits, a.alpha, a.ab_fp8 = 1, 1, 1, 1.0, 1
    return a


def run_fp8(c, what=""):
    """One row of an fp8 table: c = dict(M, N, K, batch, bmode b1|shared, alpha, adev (the value behind alpha_dev), bias,
    resid, stats, fp8 (0: the bf16 instantiation, MC_GEMM_256=2 only), A / B (operands given by the caller, fp64)).
    y [nb, M, N] = alpha * adev * A [nb, M, K] . B [nbB, N, K]^T (+ bias) (+ R)."""
    lib = L.load()
    lib.mc_gemm256_stat_rows.argtypes, lib.mc_gemm256_stat_rows.restype = [C.POINTER(L.GemmArgs)], C.c_int
    M, N, K, nb = c["M"], c["N"], c["K"], c.get("batch", 1)
    fp8, alpha, adev = c.get("fp8", 1), c.get("alpha", 1.0), c.get("adev")
    bmode = c.get("bmode", "b1")
    what = what or f"fp8 {nb}x{M}x{N}x{K} {c.get('path', '')}"
    seed = c.get("seed", 7) * 1000
    A = c["A"] if "A" in c else pm1(nb, M, K, seed=seed + 1)
    Bs = c["B"] if "B" in c else pm1(nb if bmode == "b1" else 1, N, K, seed=seed + 2)
    acc = A @ Bs.transpose(-1, -2)                                # ("shared": broadcast over the batch)
    assert float(acc.abs().max()) < 2 ** 24
    y = alpha * (adev if adev is not None else 1.0) * acc
    keep = []
    bias = None
    if c.get("bias"):
        bias = pick((-4.0, -2.0, 2.0, 4.0), nb, N + 4, seed=seed + 7)          # one row per batch element, bias_stride1 = N + 4
        y = y + bias[:, None, :N]
    exact16(y, what + " (before the residual)")
    Rr = None
    if c.get("resid"):
        Rr = pick((-2.0, 0.0, 2.0), 1, M, N, seed=seed + 9)
        y = exact16(y + Rr[0], what)
    if c.get("stats"):
        exact_stats(y, what)
    ref = y
    if fp8:
        a_buf, b_buf, pad = store8(A, extra=2), store8(Bs), 16
    else:
        a_buf, b_buf, pad = store16(A, extra=2), store16(Bs), 8
    a = fp8_args(M, N, K, K + pad, K + pad, a_buf.data_ptr(), b_buf.data_ptr())
    a.ab_fp8, a.batch, a.alpha = fp8, nb, alpha
    a.sA1, a.sB1 = (M + 2) * (K + pad), (N + 1) * (K + pad) if bmode == "b1" else 0
    if adev is not None:
        ad = scalar(adev)
        a.alpha_dev = ad.data_ptr()
        keep.append(ad)
    if bias is not None:
        b32 = bias.float().contiguous()
        a.bias, a.bias_stride1 = b32.data_ptr(), N + 4
        keep.append(b32)
    if Rr is not None:
        r_buf = store16(Rr, pad=16)
        a.R, a.ldr = r_buf.data_ptr(), N + 16
    for rep, mode in enumerate(("2", "0") if fp8 else ("2", "2")):
        with routes(nt=mode):
            g, ldc, s1, _ = guard2d(M, N, BF, nb, 1)
            a.C, a.ldc, a.sC1 = g.ptr(), ldc, s1
            part = None
            if c.get("stats"):
                rows = lib.mc_gemm_stat_rows(C.byref(a))
                assert rows == lib.mc_gemm256_stat_rows(C.byref(a)) == nb * ((M + 255) // 256), (what, rows)
                part = nan_rows(rows, 2, N)
                a.stat_partials = part.data_ptr()
            assert lib.mc_gemm_tile_config(C.byref(a)) == 256, f"{what}: MC_GEMM_256={mode} routes away from the 256 kernel"
            assert not lib.mc_gemm256_tn_eligible(C.byref(a)), what
            L.call("mc_gemm_bf16", C.byref(a), ops._st())
        got = g.get()
        g.check(f"{what} rep {rep}")
        assert torch.equal(got, ref), (f"{what} rep {rep} (MC_GEMM_256={mode}): {int((got != ref).sum())} of {ref.numel()} elements "
                                       f"differ, first at {(got != ref).nonzero()[0].tolist()}")
        if part is not None:
            check_rows_written(part, rows, what + " stat_partials")
            assert torch.equal(part[:rows].to(F64), block_sums(ref)), f"{what} rep {rep}: statistics partials differ from the fp64 block sums"


# K: one chunk; a ragged single tile; one full tile; a full tile plus one chunk; two full tiles plus one chunk; four full tiles
@pytest.mark.parametrize("K", [16, 112, 128, 144, 272, 512])
@pytest.mark.parametrize("N", [8, 256, 264])
@pytest.mark.parametrize("M", [8, 256, 264])
def test_fp8_gemm_ragged_tiles(M, N, K):
    """one and two tiles per dimension, full and ragged; sums of an even count of +-1 stay representable up to 512"""
    run_fp8(dict(M=M, N=N, K=K, seed=K + M + N))


@pytest.mark.parametrize("alpha", [1.0, 2.0])
@pytest.mark.parametrize("adev", [0.5, 2.0, 2.0 ** -10])
def test_fp8_gemm_alpha_dev(adev, alpha):
    """the kernel applies alpha * alpha_dev[0]"""
    run_fp8(dict(M=264, N=264, K=144, alpha=alpha, adev=adev, path=f"alpha {alpha} x alpha_dev {adev}"))


@pytest.mark.parametrize("adev", [0.5, 2.0, 2.0 ** -10])
def test_bf16_gemm256_alpha_dev(adev):
    """alpha_dev on the bf16 instantiation of the same kernel (ab_fp8 = 0, MC_GEMM_256=2)"""
    run_fp8(dict(fp8=0, M=264, N=264, K=72, alpha=2.0, adev=adev, path=f"bf16 operands, alpha 2 x alpha_dev {adev}"))


FP8_CASES = [
    dict(path="bias + residual (ldr != ldc) + alpha 2", M=264, N=264, K=80, bias=1, resid=1, alpha=2.0),
    dict(path="alpha 0.5", M=264, N=264, K=80, alpha=0.5),
    dict(path="stats, 2 x 2 tiles", M=264, N=264, K=144, stats=1),
    dict(path="stats + residual, ragged single tile", M=8, N=264, K=80, stats=1, resid=1),
    dict(path="batched, one weight matrix per batch element, stats + bias_stride1", M=264, N=264, K=80, batch=3, stats=1, bias=1),
    dict(path="batched, shared weight", M=300, N=8, K=144, batch=3, bmode="shared"),
    dict(path="520 items on 256 workgroups: second and third item per workgroup", M=300, N=264, K=80, batch=130),
    dict(path="520 items + stats", M=300, N=264, K=80, batch=130, stats=1),
]


@pytest.mark.parametrize("case", FP8_CASES, ids=_id)
def test_fp8_gemm_paths(case):
    run_fp8(case)


@pytest.mark.parametrize("M,N,K", [(16, 8, 16), (300, 264, 144), (300, 40, 272)])
def test_fp8_gemm_one_hot_rows_pick_columns_of_b(M, N, K):
    """A[m, k] = delta(k, m mod K) and B of small integers: y[m, :] is B[:, m mod K] exactly, whatever the sums' parity --
    this pins the order of k inside the two 8-byte halves of a fragment"""
    m = torch.arange(M, device=DEV)
    A = torch.zeros(1, M, K, device=DEV, dtype=F64)
    A[0, m, m % K] = 1.0
    ints = tuple(float(s * v) for v in range(1, 9) for s in (1, -1))
    B = pick(ints, 1, N, K, seed=K)
    cols = B[0].T                                                 # [K, N]: row k is what a one-hot row at k must return
    assert len({tuple(r) for r in cols.tolist()}) == K, "two k positions that cannot be told apart"
    assert torch.equal(A[0] @ B[0].T, cols[m % K])
    run_fp8(dict(M=M, N=N, K=K, A=A, B=B, path="one-hot A"))


def _reject_case(**kw):
    """a valid fp8 problem (264 x 40 x 32, operands with room for every leading dimension tried), then the changes in kw"""
    M, N, K = 264, 40, 32
    a_buf = torch.full(((M + 8) * 64,), ONE, dtype=torch.uint8, device=DEV)
    b_buf = torch.full(((M + 8) * 64,), ONE, dtype=torch.uint8, device=DEV)
    a = fp8_args(M, N, K, 48, 48, a_buf.data_ptr(), b_buf.data_ptr())
    for k, v in kw.items():
        setattr(a, k, v)
    return a, (a_buf, b_buf)


REJECTED = [
    ("c_f32", dict(c_f32=1)),
    ("a_kmajor and b_kmajor", dict(a_kmajor=1, b_kmajor=1)),
    ("a_kmajor and b_kmajor, fp32 output", dict(a_kmajor=1, b_kmajor=1, c_f32=1)),
    ("b_kmajor", dict(b_kmajor=1)),
    ("a_kmajor", dict(a_kmajor=1)),
    ("nb2 = 2", dict(batch=2, nb2=2)),
    ("splits = 2", dict(splits=2)),
    ("splits = 2, fp32 output, workspace", dict(splits=2, c_f32=1, ws=1)),
    ("splits = 2, fp32 output, atomics", dict(splits=2, c_f32=1, c_atomic=1)),
    ("K = 24", dict(K=24)),
    ("K = 8", dict(K=8)),
    ("lda = 40", dict(lda=40)),
    ("ldb = 40", dict(ldb=40)),
    ("lda = 56", dict(lda=56)),
]


@pytest.mark.parametrize("name,change", REJECTED, ids=[_id(n) for n, _ in REJECTED])
def test_fp8_gemm_rejects(name, change):
    """ab_fp8 outside the plain NT, 16-bit output, unsplit, K / lda / ldb % 16 == 0 form: an error, and no write"""
    lib = L.load()
    change = dict(change)
    ws = torch.full((2 * 264 * 40 + 16,), float("nan"), device=DEV) if change.pop("ws", 0) else None
    a, keep = _reject_case(**change)
    if ws is not None:
        a.splitk_ws = ws.data_ptr()
    for mode in ("2", "0", "1"):
        with routes(nt=mode, tn="2"):
            g, ldc, s1, s2 = guard2d(264, 40, F32 if a.c_f32 else BF, 2, 2)
            a.C, a.ldc, a.sC1, a.sC2 = g.ptr(), ldc, s1, s2
            assert lib.mc_gemm_bf16(C.byref(a), ops._st()) != 0, f"{name} (MC_GEMM_256={mode}): accepted"
            assert lib.mc_last_error().startswith(b"gemm"), lib.mc_last_error()
        torch.cuda.synchronize()
        assert bool((g.raw == g.sent).all()), f"{name}: the output was written"
        assert ws is None or bool(torch.isnan(ws).all())
    # the same arguments without the change are a valid launch (the case tests the change, not a typo in the base)
    ok, keep2 = _reject_case()
    g, ldc, _, _ = guard2d(264, 40, BF)
    ok.C, ok.ldc = g.ptr(), ldc
    L.call("mc_gemm_bf16", C.byref(ok), ops._st())
    g.check(name)
    assert torch.equal(g.get(), torch.full((1, 264, 40), 32.0, device=DEV, dtype=F64))


@pytest.mark.parametrize("tn", ["2", "1", "0"])
def test_alpha_dev_on_a_tn_fp32_problem_is_an_error(tn):
    """a weight-gradient problem (TN, fp32 output) that carries alpha_dev must reach mc_gemm_bf16's check -- not run on the
    256 x 256 TN kernel with the factor ignored"""
    lib = L.load()
    M, N, K = 512, 512, 2048                                      # (full tiles over 2048 rows: the TN kernel's own size rule says yes)
    A, B = store16(pm1(1, K, M, seed=1)), store16(pm1(1, K, N, seed=2))
    ad = scalar(0.5)
    a = L.GemmArgs()
    a.A, a.B, a.M, a.N, a.K, a.lda, a.ldb = A.data_ptr(), B.data_ptr(), M, N, K, M + 8, N + 8
    a.a_kmajor, a.b_kmajor, a.c_f32, a.batch, a.nb2, a.splits, a.alpha = 1, 1, 1, 1, 1, 1, 1.0
    with routes(tn=tn):
        g, ldc, _, _ = guard2d(M, N, F32)
        a.C, a.ldc = g.ptr(), ldc
        if tn != "0":
            assert lib.mc_gemm256_tn_eligible(C.byref(a)), "the base problem is not one the TN kernel takes"
        a.alpha_dev = ad.data_ptr()
        assert not lib.mc_gemm256_tn_eligible(C.byref(a)), "mc_gemm256_tn_eligible accepts a problem that carries alpha_dev"
        assert lib.mc_gemm_bf16(C.byref(a), ops._st()) != 0, "alpha_dev on a TN fp32 problem was accepted"
        assert b"alpha_dev" in lib.mc_last_error(), lib.mc_last_error()
    torch.cuda.synchronize()
    assert bool((g.raw == g.sent).all()), "the output was written"


# ------------------------------------------------------------------------------------------------ ops.linear_fwd_fp8
def _pow2_operands(rows, N, K, n_w, jx, jw, seed):
    """x [rows, K] in {+-2^jx}, w [n_w, N, K] in {+-2^jw} with amax = 448 * 2^j: both scales are powers of two, the codes are
    +-1 and alpha_dev = 2^(jx + jw): nothing rounds"""
    x, w = pm1(rows, K, seed=seed) * 2.0 ** jx, pm1(n_w, N, K, seed=seed + 1) * 2.0 ** jw
    return exact16(x, "x"), exact16(w, "w"), scalar(448.0 * 2.0 ** jx), scalar(448.0 * 2.0 ** jw)


def test_linear_fwd_fp8_plain_is_exact():
    M, N, K = 264, 264, 144
    x, w, ax, aw = _pow2_operands(M, N, K, 1, 3, -2, seed=50)
    ref = exact16(x @ w[0].T, "y")
    exact_stats(ref, "y")
    for mode in ("2", "0"):
        with routes(nt=mode):
            y, part = ops.linear_fwd_fp8(x.to(BF), w[0].to(BF), amax_x=ax, amax_w=aw, stats=True)
        assert torch.equal(y.to(F64), ref), f"{int((y.to(F64) != ref).sum())} elements differ"
        assert torch.equal(part.to(F64), block_sums(ref[None]))


def test_linear_fwd_fp8_per_image_weights_is_exact():
    """the batch_w form of the gated project conv: 3 images x 300 rows, one weight matrix per image"""
    n_img, hw, N, K = 3, 300, 264, 144
    x, w, ax, aw = _pow2_operands(n_img * hw, N, K, n_img, -1, 2, seed=60)
    ref = exact16(torch.einsum("bmk,bnk->bmn", x.view(n_img, hw, K), w), "y")
    exact_stats(ref, "y")
    for mode in ("2", "0"):
        with routes(nt=mode):
            y, part = ops.linear_fwd_fp8(x.to(BF), w.to(BF), amax_x=ax, amax_w=aw, stats=True, batch_w=(n_img, hw))
        assert torch.equal(y.to(F64).view(n_img, hw, N), ref)
        assert torch.equal(part.to(F64), block_sums(ref))


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")], ids=["inf", "minus_inf", "nan"])
def test_linear_fwd_fp8_does_not_hide_a_non_finite_activation(bad):
    """one Inf / NaN in x with the amax measured on x: the row that holds it is non-finite in y"""
    M, N, K = 264, 40, 144
    x, w, _, aw = _pow2_operands(M, N, K, 1, 0, 0, seed=70)
    xb = x.to(BF)
    xb[137, 77] = bad
    y = ops.linear_fwd_fp8(xb, w[0].to(BF), amax_w=aw)
    assert not bool(torch.isfinite(y[137].float()).any()), "the row of the non-finite activation came out finite"


# ------------------------------------------------------------------------------------------------ mc_gate_weights_bf16
@pytest.mark.parametrize("n_img,N,K", [(1, 8, 8), (1, 8, 264), (3, 8, 8), (3, 24, 8), (1, 24, 264), (3, 24, 264), (3, 8, 264), (1, 32, 64),
                                       (2, 16, 128)])
def test_gate_weights_exact(n_img, N, K):
    """out[i, n, k] = w[n, k] * gate[i, k] with w in +-{0.25, 1, 4} and gates in {0.5, 1, 2}: exact; 1 .. 2376 vectors of 8 --
    fewer than a workgroup, exactly 256 and 512, and counts that are no multiple of 256"""
    vec = n_img * N * K // 8
    assert (vec % 256 == 0) == ((n_img, N, K) in ((1, 32, 64), (2, 16, 128)))
    w = exact16(pm1(N, K, seed=N + K) * pick((0.25, 1.0, 4.0), N, K, seed=N + K + 1), "w")
    gate = pick(GATES, n_img, K, seed=n_img + K)
    ref = exact16(w[None] * gate[:, None, :], "gated w")
    wb, g32 = w.to(BF).contiguous(), gate.float().contiguous()
    for rep in range(2):
        g = Guard(BF, [(16, n_img * N, K, K)], 16 + n_img * N * K + 16)
        L.call("mc_gate_weights_bf16", wb.data_ptr(), g32.data_ptr(), n_img, N, K, g.ptr(), ops._st())
        got = g.get()[0].view(n_img, N, K)
        g.check(f"gate_weights {n_img}x{N}x{K} rep {rep}")
        assert torch.equal(got, ref), f"{int((got != ref).sum())} elements differ"
    assert torch.equal(ops.gate_weights(wb, g32).to(F64), ref)
