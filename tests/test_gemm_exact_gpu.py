"""The six GEMM kernels (gemm.hip, gemm256.hip, gemm256_tn.hip, gemm_rows.hip, gemm_wgrad_rows.hip) at the smallest shapes
that reach each of their paths, on operands for which the product is EXACT.  GPU only (`pytest -m gpu`).

Method.  Every operand element is drawn from {-1, +1} (seeded).  Every product is then +-1 and every partial sum an integer
below 2^24, so fp32 accumulation is exact in ANY order -- MFMA, split-K workspace, float atomics, ordered sums -- and for a
16-bit output with K <= 256 the final rounding is exact as well (|y| <= 256; past 256 a sum of an even number of +-1 is even
and still representable up to 512).  The reference is an fp64 matmul of the same integers with plain torch and the
comparison is torch.equal: with no zero in the operands a dropped, doubled or misplaced element moves at least one output by
an odd integer, and nothing hides under a tolerance.  The exactness carries over to alpha in {0.5, 2}, integer bias /
residual / prefilled C, and gates from {0.5, 1, 2} (gate-only prologues, split_scale).  The conditions are asserted on the
reference, before the launch: it survives the round trip through the storage type (`exact16`), and column statistics stay
below 2^24 (`exact_stats`).

The BN+SiLU prologue is not exact.  Its cases keep the two bounds of test_kernels_gpu.py (1e-2 for 16-bit outputs, 2e-3 for
fp32 outputs) -- the only tolerances in this file -- applied PER OUTPUT TILE REGION (`check_regions`), each region normalised by
its own max|ref|, so an error confined to the ragged last tile is measured against that tile.

Every launch writes into a guarded buffer (`Guard`): leading dimension wider than N, rows after M, gaps between batch slices,
everything prefilled with a NaN bit pattern that must come back bit-identical outside the output.  Operand padding holds 7.0: a
read past an operand's edge that reaches the accumulators moves an output by a multiple of 7.  Statistics partials and split-K
workspaces start as NaN and must come back finite with the row count the library's query promised, and not one row more.
Each case runs twice on fresh buffers (the second launch finds the first one's LDS).

One table per kernel family; each row names the path it is there for, and the route is asserted wherever the library can be
asked (mc_gemm_tile_config, mc_gemm256_tn_eligible, ops._tn256_plan, mc_gemm_stat_rows, mc_gemm256_stat_rows,
mc_gemm_rows_blocks, mc_wgrad_rows_blocks, mc_xbwd_rows_blocks, the *_supported predicates).
"""
import ctypes as C
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16               # the 16-bit storage dtype of the loaded kernel library (bf16; f16 under MC_STORAGE=f16)
DRY = False                 # True: build every reference, assert the exactness conditions and the routes, launch nothing
F64 = torch.float64
NAN = float("nan")
GATES = (0.5, 1.0, 2.0)
TOL16, TOL32 = 1e-2, 2e-3   # test_kernels_gpu.py's bounds for 16-bit / fp32 outputs (BN+SiLU prologue cases only)


# ------------------------------------------------------------------------------------------------ helpers
def pm1(*shape, seed):
    """+-1, seeded, as fp64"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(0, 2, shape, generator=g, dtype=torch.int8).to(F64) * 2 - 1).to(DEV)


def pick(values, *shape, seed):
    """seeded draw from a small set of exactly representable values, as fp64"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.tensor(values, dtype=F64)[torch.randint(0, len(values), shape, generator=g)].to(DEV)


def gauss(*shape, seed, scale=1.0):
    """Gaussian, rounded to the storage type, as fp64 (operands of the BN+SiLU prologue cases)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(F64).to(DEV)


def exact16(t, what):
    """the exactness condition of a 16-bit tensor: it survives the round trip through the storage type"""
    assert torch.equal(t.to(BF).to(F64), t), f"{what}: not representable in {BF}"
    return t


def exact_stats(y, what):
    """column sums of |y| and y^2 below 2^24: every fp32 partial sum is then an exact integer, in any order"""
    assert float(y.abs().sum(-2).max()) < 2 ** 24 and float((y * y).sum(-2).max()) < 2 ** 24, f"{what}: sums reach 2^24"
    assert torch.equal(y, y.round()), f"{what}: statistics of non-integers"


def store16(mats, pad=8, extra=1):
    """[nb, R, C] fp64 -> 16-bit [nb, R + extra, C + pad]; the padding holds 7.0"""
    exact16(mats, "operand")
    nb, r, c = mats.shape
    t = torch.full((nb, r + extra, c + pad), 7.0, device=DEV, dtype=BF)
    t[:, :r, :c] = mats.to(BF)
    return t


class Guard:
    """A flat buffer of NaN bit patterns (0x7F81 / 0x7FC12345) in which a launch may write only `slices` =
    [(offset, rows, cols, ld)]; check() demands every other element bit-identical."""

    def __init__(self, dtype, slices, total):
        self.dtype, self.slices = dtype, slices
        two = torch.empty(0, dtype=dtype).element_size() == 2
        self.es = 2 if two else 4
        self.sent = 0x7F81 if two else 0x7FC12345
        self.raw = torch.full((total,), self.sent, dtype=torch.int16 if two else torch.int32, device=DEV)
        self.flat = self.raw.view(dtype)

    def view(self, i=0):
        off, r, c, ld = self.slices[i]
        return self.flat.as_strided((r, c), (ld, 1), off)

    def ptr(self):
        return self.flat.data_ptr() + self.slices[0][0] * self.es

    def fill(self, values):
        """prefill the output slices (accumulating launches); values [n_slices, rows, cols]"""
        for i in range(len(self.slices)):
            self.view(i).copy_(values[i].to(self.dtype))

    def get(self):
        return torch.stack([self.view(i) for i in range(len(self.slices))]).to(F64)

    def check(self, what):
        raw = self.raw.clone()
        for off, r, c, ld in self.slices:
            raw.as_strided((r, c), (ld, 1), off).fill_(self.sent)
        assert bool((raw == self.sent).all()), f"{what}: a guard element outside the output changed"


def guard2d(M, N, dtype, nb1=1, nb2=1):
    """output [nb1, nb2, M, N] with ld = N + 8 (16 bit) / N + 4 (fp32), 2 guard rows after each slice and 8 more between
    the outer batches -> (Guard, ldc, sC1, sC2)"""
    ld = N + (8 if dtype != torch.float32 else 4)
    s2 = (M + 2) * ld
    s1 = nb2 * s2 + 8 * ld
    slices = [(16 + b1 * s1 + b2 * s2, M, N, ld) for b1 in range(nb1) for b2 in range(nb2)]
    return Guard(dtype, slices, 16 + nb1 * s1 + 16), ld, s1, s2


def nan_rows(rows, *shape):
    """float32 [rows + 1, *shape] of NaN: `rows` rows for the launch and one that must stay NaN"""
    return torch.full((rows + 1,) + tuple(shape), NAN, device=DEV, dtype=torch.float32)


def check_rows_written(buf, rows, what, prefix=False):
    """the first `rows` rows finite, the extra row untouched.  prefix=True (per-workgroup workspaces of a launch that may
    start fewer workgroups than the query's cap): a non-empty prefix of whole rows finite, the rest untouched."""
    fin = torch.isfinite(buf).flatten(1)
    full, none = fin.all(1), ~fin.any(1)
    assert bool((full | none).all()), f"{what}: a partly written row"
    n = int(full.sum())
    assert bool(full[:n].all()) and 1 <= n <= rows, f"{what}: {n} rows written, not a prefix of the {rows} promised"
    assert prefix or n == rows, f"{what}: {n} rows written, {rows} promised"
    return n


def check_regions(got, ref, tm, tn, tol, what):
    """max|got - ref| <= tol * max|ref| on every tm x tn tile region of a 2-D output, each region by its own max|ref|"""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: shape / non-finite"
    M, N = ref.shape
    err, bound = [], []
    for i in range(0, M, tm):
        for j in range(0, N, tn):
            g, r = got[i:i + tm, j:j + tn], ref[i:i + tm, j:j + tn]
            err.append((g - r).abs().max())
            bound.append(tol * r.abs().max())
    err, bound = torch.stack(err), torch.stack(bound)
    bad = (err > bound).nonzero().flatten().tolist()
    assert not bad, f"{what}: regions {bad[:6]} of {len(err)}: err {err[bad[0]]:.3e} > {bound[bad[0]]:.3e}"


def _id(v):
    """test id of a table row: its path, letters and digits only"""
    return re.sub(r"[^A-Za-z0-9]+", "_", v["path"] if isinstance(v, dict) else str(v)).strip("_")


class routes:
    """MC_GEMM_256 / MC_GEMM_256TN around the launches inside (read by the library on every call)"""

    def __init__(self, nt="0", tn="0"):
        self.want = {"MC_GEMM_256": nt, "MC_GEMM_256TN": tn}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.want}
        os.environ.update(self.want)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def silu_bn64(x, scale, shift, gate_rows):
    """the prologue in fp64, rounded once to the storage type like the staged operand: silu(x*scale + shift) * gate"""
    z = x * scale.to(F64) + shift.to(F64)
    a = z * torch.sigmoid(z)
    if gate_rows is not None:
        a = a * gate_rows.to(F64)
    return a.to(BF).to(F64)


# ------------------------------------------------------------------------------------------------ tile GEMMs (mc_gemm_bf16)
def run_gemm(c, what=""):
    """One row of a tile-GEMM table: c = dict(lay nt|nn|tn, M, N, K, f32, batch (nb1, nb2), alpha, bias, resid, stats,
    max_grid_m, splits, ws, atomic, groups (rows, sub), pro (kind, rows per image), route nt|tn|None (the 256 kernels),
    gm (expected workgroup rows of the 128 family's statistics)).  Layout of the logical product per batch element:
    A [M, K] . B [K, N]; nt: A[m][k] B[n][k], nn: A[m][k] B[k][n], tn: A[k][m] B[k][n]."""
    lib = L.load()
    lay, M, N, K = c["lay"], c["M"], c["N"], c["K"]
    what = what or f"{lay} {M}x{N}x{K} {c.get('path', '')}"
    f32, (nb1, nb2) = c.get("f32", 0), c.get("batch", (1, 1))
    alpha, splits, pro = c.get("alpha", 1.0), c.get("splits", 1), c.get("pro")
    akm, bkm = lay == "tn", lay in ("nn", "tn")
    seed = c.get("seed", 7) * 1000
    bn = pro is not None and pro[0] in ("bnA", "bnB")
    nb = nb1 * nb2
    bmode = c.get("bmode", "b1" if nb2 == 1 else "b2")           # which batch index selects the B matrix
    nbB = {"b1": nb1, "b2": nb2, "shared": 1}[bmode]
    draw = (lambda *s, seed: gauss(*s, seed=seed, scale=0.7)) if bn else pm1
    A = draw(nb1, nb2, M, K, seed=seed + 1)
    Bs = draw(nbB, K, N, seed=seed + 2)
    B = (Bs[:, None] if bmode == "b1" else Bs[None]).expand(nb1, nb2, K, N)
    a = L.GemmArgs()
    keep = []
    # ---- prologue: what the kernel multiplies is (A_eff, B_eff)
    A_eff, B_eff = A, B
    if pro is not None:
        kind, rpi = pro
        a.pro_rows_per_img = rpi
        if kind in ("gateA", "bnA"):                              # pro_operand 1: A [pixel, channel], NT, 16-bit output
            n_img = (M + rpi - 1) // rpi
            gate = pick(GATES, n_img, K, seed=seed + 3) if kind == "gateA" else torch.sigmoid(gauss(n_img, K, seed=seed + 3))
            gr = gate[torch.arange(M, device=DEV) // rpi]
            a.pro_operand, a.pro_nch = 1, K
            if bn:
                sc, sh = gauss(K, seed=seed + 4, scale=0.5) + 1.0, gauss(K, seed=seed + 5, scale=0.3)
                A_eff = silu_bn64(A, sc, sh, gr)
            else:
                A_eff = exact16(A * gr, "gated A")
        elif kind in ("gateB", "bnB"):                            # pro_operand 2: B [pixel = k, channel = n], TN, fp32 output
            n_img = (K + rpi - 1) // rpi
            gate = pick(GATES, n_img, N, seed=seed + 3) if kind == "gateB" else torch.sigmoid(gauss(n_img, N, seed=seed + 3))
            gr = gate[torch.arange(K, device=DEV) // rpi]
            a.pro_operand, a.pro_nch = 2, N
            if bn:
                sc, sh = gauss(N, seed=seed + 4, scale=0.5) + 1.0, gauss(N, seed=seed + 5, scale=0.3)
                B_eff = silu_bn64(B, sc, sh, gr)
            else:
                B_eff = exact16(B * gr, "gated B")
        else:                                                     # pro_operand 3: batch = image, its gate scales the weight's k
            assert kind == "gateW" and bmode == "shared" and nb2 == 1
            gate = pick(GATES, nb1, K, seed=seed + 3)
            a.pro_operand, a.pro_nch = 3, K
            B_eff = exact16(B * gate[:, None, :, None], "gated W")
        gate32 = gate.float().contiguous()
        a.pro_gate = gate32.data_ptr()
        keep.append(gate32)
        if bn:
            sc32, sh32 = sc.float().contiguous(), sh.float().contiguous()
            a.pro_scale, a.pro_shift = sc32.data_ptr(), sh32.data_ptr()
            keep += [sc32, sh32]
    # ---- reference (fp64)
    groups = c.get("groups")
    if groups is not None:                                        # grouped split-K: partial of group g times split_scale[g][column]
        grows, sub = groups
        ng = (K + grows - 1) // grows
        sscale = pick(GATES, ng, N, seed=seed + 6)
        acc = sum((A_eff[..., g * grows:(g + 1) * grows] @ B_eff[..., g * grows:(g + 1) * grows, :]) * sscale[g]
                  for g in range(ng))
        splits = ng * sub
        ss32 = sscale.float().contiguous()
        a.split_group_rows, a.split_sub, a.split_scale = grows, sub, ss32.data_ptr()
        keep.append(ss32)
    else:
        acc = A_eff @ B_eff
    y = alpha * acc
    bias = None
    if c.get("bias"):
        bias = pick((-4.0, -2.0, 2.0, 4.0), nb1, N + 4, seed=seed + 7)      # one row per outer batch, bias_stride1 = N + 4
        y = y + bias[:, None, None, :N]
    prefill = None
    if c.get("atomic"):
        prefill = pick((-6.0, -2.0, 0.0, 2.0, 4.0), nb, M, N, seed=seed + 8)
        y = y + prefill.view(nb1, nb2, M, N)
    R = None
    if not f32:
        if not bn:
            exact16(y, what + " (before the residual)")
        if c.get("resid"):
            R = pick((-2.0, 0.0, 2.0), 1, M, N, seed=seed + 9)
            y = (y.to(BF).to(F64) if bn else y) + R[0]
        if not bn:
            exact16(y, what)
    if not bn:
        assert float(acc.abs().max()) < 2 ** 24
    if c.get("stats"):
        exact_stats(y, what)
    ref = y.reshape(nb, M, N)
    # ---- operands in device memory: 16-bit, rows padded by 8 columns of 7.0, spare rows of 7.0 between batch slices
    At = A.transpose(-1, -2) if akm else A
    ra, ca = At.shape[-2:]
    a_buf = store16(At.reshape(nb1, nb2 * ra, ca), extra=2)
    Bt = Bs if bkm else Bs.transpose(-1, -2)
    rb, cb = Bt.shape[-2:]
    b_buf = store16(Bt.contiguous())
    a.A, a.B = a_buf.data_ptr(), b_buf.data_ptr()
    a.M, a.N, a.K = M, N, K
    a.lda, a.ldb = ca + 8, cb + 8
    a.a_kmajor, a.b_kmajor, a.c_f32, a.c_atomic, a.splits = int(akm), int(bkm), f32, int(bool(c.get("atomic"))), splits
    a.batch, a.nb2 = nb, nb2
    a.sA1, a.sA2 = (nb2 * ra + 2) * (ca + 8), ra * (ca + 8)
    sb = (rb + 1) * (cb + 8)
    a.sB1, a.sB2 = {"b1": (sb, 0), "b2": (0, sb), "shared": (0, 0)}[bmode]
    a.alpha, a.max_grid_m = alpha, c.get("max_grid_m", 0)
    if bias is not None:
        b32 = bias.float().contiguous()
        a.bias, a.bias_stride1 = b32.data_ptr(), N + 4
        keep.append(b32)
    if R is not None:
        r_buf = store16(R, pad=16)
        a.R, a.ldr = r_buf.data_ptr(), N + 16
    with routes(nt="2" if c.get("route") == "nt" else "0", tn="2" if c.get("route") == "tn" else "0"):
        for rep in range(2):
            g, ldc, s1, s2 = guard2d(M, N, torch.float32 if f32 else BF, nb1, nb2)
            if prefill is not None:
                g.fill(prefill)
            a.C, a.ldc, a.sC1, a.sC2 = g.ptr(), ldc, s1, s2
            ws = None
            if splits > 1 and c.get("ws", 1):
                ws = torch.full((splits * M * N + 16,), NAN, device=DEV, dtype=torch.float32)
                a.splitk_ws = ws.data_ptr()
            part = None
            if c.get("stats"):
                rows = lib.mc_gemm_stat_rows(C.byref(a))         # (the query wants the launch's own argument block)
                if c.get("route") == "nt":
                    lib.mc_gemm256_stat_rows.argtypes, lib.mc_gemm256_stat_rows.restype = [C.POINTER(L.GemmArgs)], C.c_int
                    assert rows == lib.mc_gemm256_stat_rows(C.byref(a)) == nb * ((M + 255) // 256), (what, rows)
                else:
                    assert rows == nb * c["gm"], (what, rows, c["gm"])
                part = nan_rows(rows, 2, N)
                a.stat_partials = part.data_ptr()
            # ---- the route
            assert lib.mc_gemm_tile_config(C.byref(a)) == (256 if c.get("route") == "nt" else 128), what
            assert bool(lib.mc_gemm256_tn_eligible(C.byref(a))) == (c.get("route") == "tn"), what
            if DRY:
                return
            L.call("mc_gemm_bf16", C.byref(a), ops._st())
            got = g.get()
            g.check(f"{what} rep {rep}")
            if bn:
                for z in range(nb):
                    check_regions(got[z], ref[z], 128, 128 if N > 64 else (64 if N > 32 else 32), TOL32 if f32 else TOL16,
                                  f"{what} rep {rep} batch {z}")
            else:
                assert torch.equal(got, ref), (f"{what} rep {rep}: {int((got != ref).sum())} of {ref.numel()} elements differ, "
                                               f"first at {(got != ref).nonzero()[0].tolist()}")
            if ws is not None:
                assert bool(torch.isfinite(ws[:splits * M * N]).all()), f"{what}: a split-K partial tile was not written"
                assert bool(torch.isnan(ws[splits * M * N:]).all()), f"{what}: write past the split-K workspace"
            if part is not None:
                check_rows_written(part, rows, what + " stat_partials")
                p64 = part[:rows].to(F64).view(nb, rows // nb, 2, N)
                bm = 256 if c.get("route") == "nt" else 128
                gm = rows // nb
                mt = (M + bm - 1) // bm
                blk = torch.zeros(nb, gm, 2, N, device=DEV, dtype=F64)     # workgroup row r owns the row blocks r, r + gm, ...
                for t in range(mt):
                    yb = ref[:, t * bm:(t + 1) * bm]
                    blk[:, t % gm, 0] += yb.sum(1)
                    blk[:, t % gm, 1] += (yb * yb).sum(1)
                assert torch.equal(p64, blk), f"{what} rep {rep}: statistics partials differ from the fp64 block sums"


# The 128-row tile family (gemm.hip; MC_GEMM_256 = 0 and MC_GEMM_256TN = 0 around the launch).  Its tile cannot be queried;
# dispatch_tile's rule is: N <= 32 -> 128 x 32 tiles, N <= 64 -> 128 x 64, else 128 x 128; K <= 48 -> BK = 32, else BK = 64;
# plain NT / TN operands with N > 64 and K > 48 take the direct-to-LDS form, everything else is register-staged.
#   K (k-contiguous operands, K % 8 == 0): 24 / 40 = BK 32, one ragged tile / two tiles; 56 = one ragged tile of 64;
#   136 = three tiles with a ragged tail; 192 = full tiles only.  TN (both k-major: any K): also 1, 65, 137, which end inside
#   a tile.  M: 1, 127, 128, 129, 300 (TN: the contiguous extent of A, multiples of 8: 8, 120, 128, 136, 296).
FORMS = [("nt", 0), ("nt", 1), ("nn", 0), ("nn", 1), ("tn", 1), ("tn", 0)]
K_KC, K_KM = (24, 40, 56, 136, 192), (1, 24, 40, 65, 137, 192)
M_KC, M_KM = (1, 127, 128, 129, 300), (8, 120, 128, 136, 296)


@pytest.mark.parametrize("N", [24, 40, 136])
@pytest.mark.parametrize("lay,f32", FORMS)
def test_tile128_layouts_widths_and_k_depths(lay, f32, N):
    """every layout x output type mc_gemm_bf16 accepts, at the three tile widths, both K-tile depths, ragged and full M"""
    for K in (K_KM if lay == "tn" else K_KC):
        for M in (M_KM if lay == "tn" else M_KC):
            run_gemm(dict(lay=lay, f32=f32, M=M, N=N, K=K, seed=K + M))


MS = 5 * 128 + 17       # 6 row blocks, the last one ragged
TILE128_CASES = [
    dict(path="persistent stream: 1 workgroup row walks 6 row blocks", lay="nt", M=MS, N=136, K=72, max_grid_m=1),
    dict(path="persistent stream: 2 workgroup rows", lay="nt", M=MS, N=136, K=72, max_grid_m=2),
    dict(path="persistent stream: 3 workgroup rows, narrow register-staged tiles", lay="nt", M=MS, N=40, K=40, max_grid_m=3),
    dict(path="persistent stream + stats, 1 row", lay="nt", M=MS, N=136, K=72, max_grid_m=1, stats=1, gm=1),
    dict(path="persistent stream + stats, 2 rows", lay="nt", M=MS, N=136, K=72, max_grid_m=2, stats=1, gm=2),
    dict(path="persistent stream + stats, 3 rows, BK = 32", lay="nt", M=MS, N=24, K=40, max_grid_m=3, stats=1, gm=3),
    dict(path="persistent stream, TN fp32", lay="tn", f32=1, M=MS + 7, N=136, K=137, max_grid_m=2),
    dict(path="stats, default grid: one row block per workgroup", lay="nt", M=300, N=136, K=136, stats=1, gm=3),
    dict(path="row-block XCD remap: gm = 18 >= 16, grid.y padded to 24", lay="nt", M=17 * 128 + 5, N=136, K=72),
    dict(path="row-block XCD remap + stats", lay="nt", M=17 * 128 + 5, N=136, K=72, stats=1, gm=18),
    dict(path="XCD remap, mtiles = 42 >= 2 gm: gm 20 rounded down to 16", lay="nt", M=41 * 128 + 5, N=136, K=72, max_grid_m=20),
    dict(path="XCD remap, gm 20 -> 16, stats", lay="nt", M=41 * 128 + 5, N=136, K=72, max_grid_m=20, stats=1, gm=16),
    dict(path="split-K workspace, 16 splits (split XCD remap), 6 K tiles: 10 empty splits", lay="tn", f32=1, M=136, N=40, K=337,
         splits=16),
    dict(path="split-K workspace, 16 splits, direct-to-LDS tiles", lay="tn", f32=1, M=136, N=136, K=337, splits=16),
    # (plain splits are cut at whole K tiles: the seam inside a tile is the END of the last non-empty range; the grouped
    # cases below cut at multiples of 70 rows, inside K tiles on both sides)
    dict(path="split-K workspace, 2 splits, second one a ragged K tile", lay="tn", f32=1, M=136, N=136, K=137, splits=2),
    dict(path="split-K workspace, 3 splits, last range ends inside a tile", lay="tn", f32=1, M=40, N=24, K=161, splits=3),
    dict(path="split-K workspace, NT fp32 output", lay="nt", f32=1, M=129, N=40, K=136, splits=2),
    dict(path="split-K, c_atomic, no workspace, prefilled C", lay="tn", f32=1, M=136, N=136, K=137, splits=2, ws=0, atomic=1),
    dict(path="split-K, c_atomic, no workspace, 3 splits, narrow tiles", lay="tn", f32=1, M=40, N=24, K=161, splits=3, ws=0,
         atomic=1),
    dict(path="split-K workspace accumulated into a prefilled C (c_atomic + workspace)", lay="tn", f32=1, M=136, N=40, K=137,
         splits=2, atomic=1),
    dict(path="grouped split-K + split_scale: 3 groups of 70 rows, 2 sub-splits", lay="tn", f32=1, M=136, N=136, K=210,
         groups=(70, 2)),
    dict(path="grouped split-K, narrow tiles, last group cut short", lay="tn", f32=1, M=40, N=24, K=200, groups=(70, 2)),
    dict(path="grouped split-K accumulated into a prefilled C", lay="tn", f32=1, M=136, N=40, K=210, groups=(70, 2), atomic=1),
    dict(path="batch 2 x 3 (nb2 > 1), distinct strides on A, B, C", lay="nt", f32=1, M=129, N=40, K=72, batch=(2, 3)),
    dict(path="batch 2 x 3, NN 16-bit output (the P.V form)", lay="nn", M=65, N=136, K=72, batch=(2, 3)),
    dict(path="batch 2 x 2, TN 16-bit output (the dV form)", lay="tn", M=72, N=40, K=65, batch=(2, 2)),
    dict(path="bias with bias_stride1 + alpha 0.5, batched fp32 (the Q.K^T form)", lay="nt", f32=1, M=65, N=72, K=72,
         batch=(3, 2), bias=1, alpha=0.5),
    dict(path="bias + alpha 2, 16-bit output", lay="nt", M=129, N=136, K=56, bias=1, alpha=2.0),
    dict(path="alpha 0.5, 16-bit output (half-integers)", lay="nn", M=129, N=40, K=72, alpha=0.5),
    dict(path="residual with ldr != ldc + bias", lay="nt", M=300, N=136, K=136, resid=1, bias=1),
    dict(path="residual + stats, narrow tiles", lay="nt", M=129, N=24, K=40, resid=1, stats=1, gm=2),
    dict(path="gate-only prologue on A (pro_operand 1)", lay="nt", M=300, N=136, K=72, pro=("gateA", 70)),
    dict(path="gate-only prologue on A, narrow tiles, BK = 32", lay="nt", M=129, N=24, K=40, pro=("gateA", 50)),
    dict(path="gate-only prologue on B (pro_operand 2)", lay="tn", f32=1, M=136, N=136, K=137, pro=("gateB", 50)),
    dict(path="gate-only prologue on B + split-K", lay="tn", f32=1, M=40, N=40, K=200, pro=("gateB", 70), splits=2),
    dict(path="per-batch weight gate (pro_operand 3)", lay="nt", M=129, N=136, K=72, batch=(3, 1), bmode="shared",
         pro=("gateW", 0)),
    dict(path="per-batch weight gate, narrow tiles + stats", lay="nt", M=129, N=40, K=40, batch=(3, 1), bmode="shared",
         pro=("gateW", 0), stats=1, gm=2),
    dict(path="BN+SiLU+gate prologue on A, ragged M / N / K (per-region bound)", lay="nt", M=300, N=136, K=72, pro=("bnA", 70)),
    dict(path="BN+SiLU+gate prologue on A, narrow tiles (per-region bound)", lay="nt", M=129, N=40, K=40, pro=("bnA", 50)),
    dict(path="BN+SiLU+gate prologue on B, ragged M / N / K (per-region bound)", lay="tn", f32=1, M=136, N=136, K=137,
         pro=("bnB", 50)),
    dict(path="BN+SiLU+gate prologue on B, narrow tiles + split-K (per-region bound)", lay="tn", f32=1, M=40, N=40, K=300,
         pro=("bnB", 70), splits=2),
]


@pytest.mark.parametrize("case", TILE128_CASES, ids=_id)
def test_tile128_paths(case):
    run_gemm(case)


# The 256 x 256 NT kernel (gemm256.hip; MC_GEMM_256 = 2: whenever the layout allows; mc_gemm_tile_config must say 256).
@pytest.mark.parametrize("K", [8, 64, 72, 136, 256])
def test_gemm256_nt_ragged_tiles(K):
    """one and two tiles per dimension, full and ragged: M, N in {8, 256, 264}; K from one chunk to four full K tiles"""
    for M in (8, 256, 264):
        for N in (8, 256, 264):
            run_gemm(dict(lay="nt", route="nt", M=M, N=N, K=K, seed=K + M + N))


GEMM256_CASES = [
    dict(path="bias + residual (ldr != ldc) + alpha 2", M=264, N=264, K=72, bias=1, resid=1, alpha=2.0),
    dict(path="alpha 0.5", M=264, N=264, K=72, alpha=0.5),
    dict(path="stats, 2 x 2 tiles", M=264, N=264, K=136, stats=1),
    dict(path="stats + residual, ragged single tile", M=8, N=264, K=72, stats=1, resid=1),
    dict(path="batched, one weight matrix per batch element, stats + bias_stride1", M=264, N=264, K=72, batch=(3, 1), stats=1,
         bias=1),
    dict(path="batched, shared weight", M=300, N=8, K=136, batch=(3, 1), bmode="shared"),
    dict(path="520 items on 256 workgroups: second and third item per workgroup", M=300, N=264, K=72, batch=(130, 1)),
    dict(path="520 items + stats", M=300, N=264, K=72, batch=(130, 1), stats=1),
]


@pytest.mark.parametrize("case", GEMM256_CASES, ids=_id)
def test_gemm256_nt_paths(case):
    run_gemm(dict(case, lay="nt", route="nt"))


def test_gemm256_nt_past_the_non_temporal_store_threshold():
    """batch * M * N * 2 >= 128 MiB takes the non-temporal stores: 8200 x 8200 x 72 writes 134.5 MB, ragged on both edges
    (33 x 33 tiles: every workgroup takes 4-5 items).  One launch; compared in row blocks so that the fp64 reference never
    holds more than 1025 x 8200 elements."""
    lib = L.load()
    M = N = 8200
    K = 72
    assert M * N * 2 >= 128 << 20
    x, w = pm1(1, M, K, seed=31), pm1(1, N, K, seed=32)
    xb, wb = store16(x), store16(w)
    a = L.GemmArgs()
    a.A, a.B, a.M, a.N, a.K, a.lda, a.ldb = xb.data_ptr(), wb.data_ptr(), M, N, K, K + 8, K + 8
    a.batch, a.nb2, a.splits, a.alpha = 1, 1, 1, 1.0
    with routes(nt="2"):
        g, ldc, s1, s2 = guard2d(M, N, BF)
        a.C, a.ldc = g.ptr(), ldc
        assert lib.mc_gemm_tile_config(C.byref(a)) == 256
        for r0 in range(0, M, 1025):                              # the exactness condition, block by block
            exact16(x[0, r0:r0 + 1025] @ w[0].T, "reference block")
        if DRY:
            return
        L.call("mc_gemm_bf16", C.byref(a), ops._st())
    g.check("non-temporal stores")
    got = g.view()
    for r0 in range(0, M, 1025):
        ref = x[0, r0:r0 + 1025] @ w[0].T
        blk = got[r0:r0 + 1025].to(F64)
        assert torch.equal(blk, ref), f"rows {r0}..: {int((blk != ref).sum())} elements differ"


# The 256 x 256 TN kernel (gemm256_tn.hip; MC_GEMM_256TN = 2; mc_gemm256_tn_eligible must say yes): dW [N, K] = dY [rows, N]^T .
# X [rows, K], so the product's (M, N, K) is (N of dW, K of dW, rows).
@pytest.mark.parametrize("rows", [1, 65, 137, 1000])
@pytest.mark.parametrize("n_out,k_out", [(8, 8), (8, 264), (264, 8), (264, 264)])
def test_gemm256_tn_ragged_tiles_and_splits(n_out, k_out, rows):
    """ragged output tiles, reductions that end inside a K tile, the planned split count and forced counts of 2 and 16
    (most of the 16 ranges empty), accumulation into a prefilled dW"""
    lib = L.load()
    with routes(tn="2"):
        plan = ops._tn256_plan(n_out, k_out, rows, n_out + 8, k_out + 8)
    assert plan >= 1 and plan == lib.mc_gemm256_tn_splits(n_out, k_out, rows, 0)
    base = dict(lay="tn", f32=1, route="tn", M=n_out, N=k_out, K=rows, seed=rows + n_out)
    for splits in sorted({plan, 2, 16}):
        run_gemm(dict(base, splits=splits, path=f"{splits} splits"))
        if splits > 1:
            run_gemm(dict(base, splits=splits, atomic=1, path=f"{splits} splits, accumulate"))


@pytest.mark.parametrize("n_out,k_out", [(8, 264), (264, 264)])
def test_gemm256_tn_grouped_gates(n_out, k_out):
    """the grouped form: reduction cut every 70 rows (inside K tiles), gates from {0.5, 1, 2} applied when the partials are
    combined; the planned sub-split count and a forced 2; a last group that is cut short; accumulate"""
    lib = L.load()
    rows = 3 * 70
    with routes(tn="2"):
        plan = ops._tn256_plan(n_out, k_out, rows, n_out + 8, k_out + 8, group_rows=70)
    assert plan >= 1 and plan == lib.mc_gemm256_tn_splits(n_out, k_out, rows, 70)
    base = dict(lay="tn", f32=1, route="tn", M=n_out, N=k_out, seed=n_out)
    for sub in sorted({plan, 2}):
        run_gemm(dict(base, K=rows, groups=(70, sub), path=f"grouped, {sub} sub-splits"))
        run_gemm(dict(base, K=rows - 9, groups=(70, sub), path=f"grouped, {sub} sub-splits, short last group"))
        run_gemm(dict(base, K=rows, groups=(70, sub), atomic=1, path=f"grouped, {sub} sub-splits, accumulate"))


# ------------------------------------------------------------------------------------------------ row-streaming kernels
ROWS_M = (1, 15, 16, 17, 63, 65, 100, 257)     # fewer 16-row groups than waves, M < 16, M % 16 != 0, fewer iterations than the
#                                                prefetch depth; 257 rows = 17 groups on 5 workgroups


def run_gemm_rows(M, N, K, opt, seed):
    """mc_gemm_rows_bf16 through its own argument block: y [M, N] = pro(x) [M, K] . w [N, K]^T (+ residual + bias), 16-bit.
    opt: plain | stats | resid | bn | bngate"""
    lib = L.load()
    what = f"gemm_rows {M}x{N}x{K} {opt}"
    assert lib.mc_gemm_rows_supported(N, K), what
    bn = opt in ("bn", "bngate")
    x = gauss(1, M, K, seed=seed, scale=0.7) if bn else pm1(1, M, K, seed=seed)
    w = pm1(1, N, K, seed=seed + 1)
    a = L.GemmRowsArgs()
    keep = []
    x_eff = x[0]
    if bn:
        rpi = 16                                                  # M % 16 != 0: the last image is cut short
        n_img = (M + rpi - 1) // rpi
        sc, sh = gauss(K, seed=seed + 2, scale=0.5) + 1.0, gauss(K, seed=seed + 3, scale=0.3)
        gate = torch.sigmoid(gauss(n_img, K, seed=seed + 4)) if opt == "bngate" else None
        x_eff = silu_bn64(x[0], sc, sh, None if gate is None else gate[torch.arange(M, device=DEV) // rpi])
        keep = [sc.float().contiguous(), sh.float().contiguous()] + ([gate.float().contiguous()] if gate is not None else [])
        a.pro_scale, a.pro_shift, a.pro_rows_per_img = keep[0].data_ptr(), keep[1].data_ptr(), rpi
        if gate is not None:
            a.pro_gate = keep[2].data_ptr()
    y = x_eff @ w[0].T
    if not bn:
        exact16(y, what + " (product)")
    if opt == "stats":
        exact_stats(y, what)
    ref = y
    if opt == "resid":                                            # residual + bias, added after the product was rounded
        R = pick((-2.0, 0.0, 2.0), 1, M, N, seed=seed + 5)
        bias = pick((-4.0, -2.0, 2.0, 4.0), N, seed=seed + 6)
        ref = exact16(y + R[0] + bias, what)
        r_buf, b32 = store16(R, pad=16), bias.float().contiguous()
        a.R, a.ldr, a.bias = r_buf.data_ptr(), N + 16, b32.data_ptr()
    xb, wb = store16(x), store16(w)
    a.X, a.M, a.K, a.ldx = xb.data_ptr(), M, K, K + 8
    a.W, a.N, a.ldw = wb.data_ptr(), N, K + 8
    for rep in range(2):
        g, ldc, _, _ = guard2d(M, N, BF)
        a.C, a.ldc = g.ptr(), ldc
        blocks = lib.mc_gemm_rows_blocks(C.byref(a))
        groups = (M + 15) // 16
        ntiles = (N + 127) // 128 if N > 256 else 1
        assert blocks == max(1, (groups + 3) // 4), (what, blocks)     # 4 waves per workgroup, one 16-row group each at least
        part = None
        if opt == "stats":
            part = nan_rows(blocks, 2, N)
            a.stat_partials = part.data_ptr()
        if DRY:
            return
        L.call("mc_gemm_rows_bf16", C.byref(a), ops._st())
        got = g.get()[0]
        g.check(f"{what} rep {rep}")
        if bn:
            check_regions(got, ref, 16, 128 if ntiles > 1 else N, TOL16, f"{what} rep {rep}")
        else:
            assert torch.equal(got, ref), f"{what} rep {rep}: {int((got != ref).sum())} of {ref.numel()} elements differ"
        if part is not None:
            check_rows_written(part, blocks, what + " stat_partials")
            s = part[:blocks].to(F64).sum(0)
            assert torch.equal(s[0], y.sum(0)) and torch.equal(s[1], (y * y).sum(0)), f"{what} rep {rep}: column statistics"


# launch_rows_e's register layouts: RG = 4 (64 rows per iteration: at most 2 column fragments and K <= 64), RG = 1 (16 rows: N >= 96
# or K > 256), RG = 2 (32 rows: the rest); N > 256: 128-column tiles, ntiles workgroups per row range
@pytest.mark.parametrize("N,K,layout", [(24, 24, "RG = 4, KC = 1"), (32, 56, "RG = 4, KC = 2"), (40, 72, "RG = 2, KC = 4"),
                                        (96, 40, "RG = 1 (6 column fragments)"), (40, 384, "RG = 1 (K > 256, KC = 12)"),
                                        (264, 40, "three 128-column tiles")], ids=_id)
def test_gemm_rows_few_rows(N, K, layout):
    """the row-streaming forward at 1 .. 257 rows: plain, statistics (exact), residual + bias, the data gradient through the
    transposed weight (the same kernel at (K, N)), the BN+SiLU(+gate) prologue with 16 rows per image (per-region bound)"""
    lib = L.load()
    for M in ROWS_M:
        for i, opt in enumerate(("plain", "stats", "resid", "bn", "bngate")):
            run_gemm_rows(M, N, K, opt, seed=M * 10 + i)
        if lib.mc_gemm_rows_supported(K, N):
            run_gemm_rows(M, K, N, "resid", seed=M * 10 + 7)      # dx [M, K] = dy [M, N] . w_t [K, N]^T + residual


def _wgrad_args(dy_b, x_b, M, N, K):
    a = L.WgradRowsArgs()
    a.dY, a.N, a.lddy = dy_b.data_ptr(), N, N + 8
    a.X, a.K, a.ldx, a.M = x_b.data_ptr(), K, K + 8, M
    return a


def _wgrad_out(N, K, prefill=None):
    """dW [N, K] fp32 is contiguous: guard elements in front and behind"""
    g = Guard(torch.float32, [(16, N, K, K)], 16 + N * K + 16)
    if prefill is not None:
        g.fill(prefill)
    return g


# mc_wgrad_rows_supported's branches by (dY fragments, X fragments) per wave: both <= 4; up to 6 x 4; up to 4 x 6; and the two
# instantiations with the dY slot count as a template constant, (40, 240) and (64, 384)
@pytest.mark.parametrize("N,K,branch", [(24, 24, "1 x 1 fragments"), (144, 24, "3 x 2"), (16, 96, "1 x 2, X the wider operand"),
                                        (40, 240, "3 x 4 with 2 dY slots"), (64, 384, "4 x 6 with 1 dY slot"),
                                        (384, 64, "6 x 4"), (240, 64, "4 x 4"), (320, 24, "5 x 2"), (16, 384, "1 x 6")],
                         ids=_id)
def test_wgrad_rows_few_rows(N, K, branch):
    """the streaming weight gradient at 1 .. 257 rows: plain and accumulate (exact), BN+SiLU+gate prologue on X (bound)"""
    lib = L.load()
    assert lib.mc_wgrad_rows_supported(N, K)
    for M in ROWS_M:
        what = f"wgrad_rows {M}x{N}x{K}"
        dy, x = pm1(1, M, N, seed=M), pm1(1, M, K, seed=M + 1)
        ref = dy[0].T @ x[0]
        pre = pick((-6.0, -2.0, 0.0, 2.0, 4.0), 1, N, K, seed=M + 2)
        rpi = 16
        n_img = (M + rpi - 1) // rpi
        xg = gauss(1, M, K, seed=M + 3, scale=0.7)
        sc, sh = gauss(K, seed=M + 4, scale=0.5) + 1.0, gauss(K, seed=M + 5, scale=0.3)
        gate = torch.sigmoid(gauss(n_img, K, seed=M + 6))
        ref_bn = dy[0].T @ silu_bn64(xg[0], sc, sh, gate[torch.arange(M, device=DEV) // rpi])
        sc32, sh32, g32 = sc.float().contiguous(), sh.float().contiguous(), gate.float().contiguous()
        dy_b, x_b, xg_b = store16(dy), store16(x), store16(xg)
        blocks = lib.mc_wgrad_rows_blocks(M)
        assert blocks == (M + 63) // 64, (what, blocks)
        for form in ("plain", "accumulate", "prologue"):
            for rep in range(2):
                a = _wgrad_args(dy_b, xg_b if form == "prologue" else x_b, M, N, K)
                g = _wgrad_out(N, K, pre if form == "accumulate" else None)
                ws = nan_rows(blocks, N, K)
                a.dW, a.ws, a.accumulate = g.ptr(), ws.data_ptr(), int(form == "accumulate")
                if form == "prologue":
                    a.pro_scale, a.pro_shift, a.pro_gate, a.pro_rows_per_img = sc32.data_ptr(), sh32.data_ptr(), g32.data_ptr(), rpi
                if DRY:
                    continue
                L.call("mc_wgrad_rows_bf16", C.byref(a), ops._st())
                got = g.get()[0]
                g.check(f"{what} {form} rep {rep}")
                check_rows_written(ws, blocks, f"{what} {form} workspace", prefix=True)
                if form == "prologue":
                    check_regions(got, ref_bn, 64, 64, TOL32, f"{what} prologue rep {rep}")
                else:
                    want = ref + pre[0] if form == "accumulate" else ref
                    assert torch.equal(got, want), f"{what} {form} rep {rep}: {int((got != want).sum())} elements differ"


# xbwd_cfg's five instantiations: the expand geometries of EfficientNet-B2 / -B5
@pytest.mark.parametrize("N,K", [(96, 16), (144, 24), (240, 40), (288, 48), (384, 64)])
def test_xbwd_rows_few_rows(N, K):
    """both gradients of an expand conv from one pass over dY, at 1 .. 257 rows: dW [N, K] = dY^T x (fp32, exact) and
    dX [M, K] = dY . wt^T with and without the residual (16 bit, exact: sums of an even number of +-1)"""
    lib = L.load()
    assert lib.mc_xbwd_rows_supported(N, K)
    for M in ROWS_M:
        what = f"xbwd_rows {M}x{N}x{K}"
        dy, x, wt = pm1(1, M, N, seed=M), pm1(1, M, K, seed=M + 1), pm1(1, K, N, seed=M + 2)
        R = pick((-2.0, 0.0, 2.0), 1, M, K, seed=M + 3)
        ref_dw = dy[0].T @ x[0]
        ref_dx = exact16(dy[0] @ wt[0].T, what + " dX")
        ref_dxr = exact16(ref_dx + R[0], what + " dX + r")
        dy_b, x_b, wt_b, r_b = store16(dy), store16(x), store16(wt), store16(R, pad=16)
        blocks = lib.mc_xbwd_rows_blocks(M)
        assert blocks == (M + 31) // 32, (what, blocks)
        for with_r in (False, True):
            for rep in range(2):
                a = _wgrad_args(dy_b, x_b, M, N, K)
                g = _wgrad_out(N, K)
                gx, lddx, _, _ = guard2d(M, K, BF)
                ws = nan_rows(blocks, N, K)
                a.dW, a.ws, a.accumulate = g.ptr(), ws.data_ptr(), 0
                if DRY:
                    continue
                L.call("mc_xbwd_rows_bf16", C.byref(a), wt_b.data_ptr(), N + 8, gx.ptr(), lddx,
                       r_b.data_ptr() if with_r else None, K + 16 if with_r else 0, ops._st())
                dw, dx = g.get()[0], gx.get()[0]
                g.check(f"{what} dW rep {rep}")
                gx.check(f"{what} dX rep {rep}")
                check_rows_written(ws, blocks, f"{what} workspace", prefix=True)
                want = ref_dxr if with_r else ref_dx
                assert torch.equal(dw, ref_dw), f"{what} r={with_r} rep {rep}: dW, {int((dw != ref_dw).sum())} elements differ"
                assert torch.equal(dx, want), f"{what} r={with_r} rep {rep}: dX, {int((dx != want).sum())} elements differ"
