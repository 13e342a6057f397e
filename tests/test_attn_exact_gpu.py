"""The fused self-attention kernels of attn.hip (resident and long bodies, padded and packed view, with and without dropout) and
the softmax kernels of bert.hip (the unfused path) against an INDEPENDENT fp64 reference at their block, chunk and sequence
seams, on operands for which the arithmetic is exact.  GPU only (`pytest -m gpu`).

Method (tests/_attn_exact_cases.py holds the tables, the builder, the references and the derivation).  Two-hot class codes make
every score 256, 128 or 0: the softmax of a row is exactly 1/m on its m in {1, 2, 4, 8} maximal keys and exactly 0 elsewhere;
sparse small-integer payloads keep ctx, dS, dQ, dK and dV dyadic rationals of a few bits, so every fp32 sum is exact in any order
and every 16-bit rounding is the identity.  The reference is the kernels' formulas in fp64 with plain torch on the CPU, the
dropout mask a host Philox4x32-10, and every comparison is torch.equal -- a key block that is dropped, doubled or taken from the
wrong chunk, a zero-filled LDS row or a neighbouring sequence's row admitted as a key, a dropout bit on the wrong (query, key)
pair in one sweep, a wrong lse entry: each moves some output by at least its last bit, and nothing hides under a tolerance.
No kernel output enters a reference.

test_exp_and_reciprocal_are_exact proves the three device facts the method rests on -- __expf(0) == 1, __expf(x <= -128) == 0,
1 / 2^k exact -- through the forward kernels themselves.  If it fails, it reports the bits seen, and the remaining cases compare
the P-dependent outputs (1/sum, ctx, dQ, dK, dV, probabilities, dS) within one unit in the last place of the storage type per
element, |got - ref| <= eps * max(|got|, |ref|) with eps = 2^-7 (bf16) / 2^-10 (f16); row maxima, guards and zero rows stay exact.

Every launch goes through L.call on buffers of its own: ctx, dqkv and lse live in flat buffers of NaN bit patterns (`Guard`, as
in test_gemm_exact_gpu.py) with guard rows in front and behind, and every element outside the promised output must come back
bit-identical (in the packed view that includes the lse entries of the alignment rows); inputs are followed by a NaN row, the
alignment rows of packed qkv and dctx hold NaN -- the kernels must never read them -- and those of ctx and dqkv must come back
exactly zero.  Each case runs forward then backward, twice on fresh buffers (the second launch finds the first one's LDS).
Rows with at most 256 keys run on the resident AND the long pair, which must also agree with each other bit for bit."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
import mammo_clip_amd.lib as L  # noqa: E402

import _attn_exact_cases as X  # noqa: E402

DEV = torch.device("cuda:0")
BF = ops.BF16
F32, F64 = torch.float32, torch.float64
EPS = 2.0 ** -7 if BF == torch.bfloat16 else 2.0 ** -10      # one unit in the last place, relative (the fallback only)
assert BF == X.ST

FWD = {("padded", "res"): "mc_attn_fwd", ("padded", "long"): "mc_attn_long_fwd",
       ("packed", "res"): "mc_attn_varlen_fwd", ("packed", "long"): "mc_attn_varlen_long_fwd"}
BWD = {k: v.replace("_fwd", "_bwd") for k, v in FWD.items()}


class Guard:
    """A flat buffer of NaN bit patterns (0x7F81 / 0x7FC12345) in which a launch may write only `slices` =
    [(offset, rows, cols, ld)]; check() demands every other element bit-identical.  (test_gemm_exact_gpu.py's helper.)"""

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
        p = self.flat.data_ptr() + self.slices[0][0] * self.es
        assert p % 16 == 0
        return p

    def get(self):
        return self.view().to(F64).cpu()

    def bits(self):
        off, r, c, ld = self.slices[0]
        return self.raw.as_strided((r, c), (ld, 1), off).cpu()

    def check(self, what):
        raw = self.raw.clone()
        for off, r, c, ld in self.slices:
            raw.as_strided((r, c), (ld, 1), off).fill_(self.sent)
        assert bool((raw == self.sent).all()), f"{what}: a guard element outside the output changed"


def rows_guard(written, cols, dtype, room=None):
    """[written, cols] contiguous rows a launch may write, 4 guard rows in front and 4 behind the `room` >= written rows the
    buffer has (packed lse: the alignment rows are part of the buffer and must stay untouched)"""
    room = written if room is None else room
    off = 4 * max(cols, 8)
    return Guard(dtype, [(off, written, cols, cols)], off + room * cols + 4 * max(cols, 8))


def dev16(t):
    """fp64 [R, C] (NaN in rows no kernel may read) -> the storage type on the device, followed by one NaN row"""
    fin = t[torch.isfinite(t).all(1)]
    assert torch.equal(fin.to(BF).to(F64), fin)
    return torch.cat([t, torch.full((1, t.shape[1]), float("nan"), dtype=F64)]).to(BF).to(DEV)


def same(got, ref, what, exact):
    """torch.equal; exact=False (the precondition failed): one unit in the last place of the storage type per element"""
    assert got.shape == ref.shape, what
    if exact:
        bad = got != ref
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {ref.numel()} elements differ from the fp64 reference, first at "
                                     f"{bad.nonzero()[0].tolist()}: {got[bad][0].item()!r} != {ref[bad][0].item()!r}")
    else:
        bad = ~((got - ref).abs() <= EPS * torch.maximum(got.abs(), ref.abs()))
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {ref.numel()} elements further than one ulp from the reference"


class Launch:
    """the device side of a case: its inputs (shared by pairs and repetitions) and forward + backward on fresh guarded outputs"""

    def __init__(self, cs, ref):
        self.cs, self.ref = cs, ref
        self.R, self.H, self.real = X.total_rows(cs), cs.nh * X.HD, sum(X.seq_lens(cs))
        self.qkv, self.dctx = dev16(ref.qkv), dev16(ref.dctx)
        if cs.view == "padded":
            assert self.R == self.real == cs.b * cs.t
            self.maskb = torch.cat([ref.maskb.flatten(), torch.full((8,), float("nan"), dtype=F64)]).to(F32).to(DEV)
            self.lse_rows = self.lse_room = cs.b * cs.nh * cs.t
        else:
            cu = torch.tensor([0] + [sum(cs.lens[:i + 1]) for i in range(cs.b)], dtype=torch.int32)
            assert int(cu[-1]) == self.real <= self.R
            self.cu = cu.to(DEV)
            order = X.order_of(cs)
            self.order = None if order is None else order.to(DEV)
            self.lse_rows, self.lse_room = self.real * cs.nh, self.R * cs.nh
        self.lse_ref = ref.lse.reshape(-1, 2)[:self.lse_rows]

    def head(self, pair):
        """the arguments between the input pointers and (alpha, p, seed, stream id)"""
        cs = self.cs
        lib = L.load()
        if cs.view == "padded":
            ok = lib.mc_attn_supported if pair == "res" else lib.mc_attn_long_supported
            assert ok(cs.t, X.HD), (cs.seam, pair)
            return (cs.b, cs.t, cs.nh)
        ok = lib.mc_attn_varlen_supported if pair == "res" else lib.mc_attn_varlen_long_supported
        assert ok(max(cs.lens), X.HD), (cs.seam, pair)
        return (cs.b, max(cs.lens), X.t_pad(cs), self.R, cs.nh)

    def forward(self, pair):
        cs = self.cs
        ctx, lse = rows_guard(self.R, self.H, BF), rows_guard(self.lse_rows, 2, F32, self.lse_room)
        ins = (self.qkv.data_ptr(), self.maskb.data_ptr()) if cs.view == "padded" else \
            (self.qkv.data_ptr(), self.cu.data_ptr(), ops._p(self.order))
        L.call(FWD[cs.view, pair], *ins, *self.head(pair), X.ALPHA, cs.p, X.SEED, X.SID, ctx.ptr(), lse.ptr(), ops._st())
        return ctx, lse

    def backward(self, pair, lse):
        cs = self.cs
        dqkv = rows_guard(self.R, 3 * self.H, BF)
        ins = (self.qkv.data_ptr(), self.maskb.data_ptr()) if cs.view == "padded" else \
            (self.qkv.data_ptr(), self.cu.data_ptr(), ops._p(self.order))
        L.call(BWD[cs.view, pair], *ins, self.dctx.data_ptr(), lse.ptr(), *self.head(pair), X.ALPHA, cs.p, X.SEED, X.SID,
               dqkv.ptr(), ops._st())
        return dqkv

    def run(self, pair, exact):
        """forward then backward, twice on fresh buffers, everything compared with the reference -> the last repetition's bits"""
        cs, ref, H = self.cs, self.ref, self.H
        for rep in range(2):
            what = f"{cs.seam} [{FWD[cs.view, pair]} / _bwd] rep {rep}"
            ctx, lse = self.forward(pair)
            dqkv = self.backward(pair, lse)
            torch.cuda.synchronize()
            for g, name in ((ctx, "ctx"), (lse, "lse"), (dqkv, "dqkv")):
                g.check(f"{what} {name}")
            got = lse.get()
            assert bool(torch.isfinite(got).all()), f"{what}: an lse entry of a real row was not written"
            same(got[:, 0], self.lse_ref[:, 0], f"{what} lse row max", True)
            same(got[:, 1], self.lse_ref[:, 1], f"{what} lse 1 / row sum", exact)
            c, d = ctx.get(), dqkv.get()
            assert not bool(c[self.real:].ne(0).any()) and not bool(d[self.real:].ne(0).any()), f"{what}: alignment rows not zero"
            same(c, ref.ctx, f"{what} ctx", exact)
            for part, name in enumerate(("dQ", "dK", "dV")):
                same(d[:, part * H:(part + 1) * H], ref.dqkv[:, part * H:(part + 1) * H], f"{what} {name}", exact)
        return ctx.bits(), lse.bits(), dqkv.bits()


# ------------------------------------------------------------------------------------------------ the precondition
@functools.lru_cache(maxsize=1)
def precondition_failures():
    """T = 32, one head, classes of 1 and 2, no dropout, no mask, forward of the resident and of the long kernel: lse must be
    (256, 1/m) and ctx the reference, exactly -> what is not exact, with the bits seen ([] if all three facts hold)"""
    cs = X.PRECONDITION
    ref = X.reference(cs)
    run = Launch(cs, ref)
    m = (1.0 / run.lse_ref[:, 1]).round().long()
    assert set(m.tolist()) == {1, 2} and set(run.lse_ref[:, 0].tolist()) == {256.0}
    out = []
    for pair in cs.pairs:
        ctx, lse = run.forward(pair)
        torch.cuda.synchronize()
        ctx.check(f"precondition [{pair}] ctx")
        lse.check(f"precondition [{pair}] lse")
        got, bits = lse.get(), lse.bits()
        if not torch.equal(got[:, 0], run.lse_ref[:, 0]):
            out.append(f"{pair}: row max is not 256: bits {sorted({hex(v & 0xFFFFFFFF) for v in bits[:, 0].tolist()})}")
        one, two = bits[m == 1, 1], bits[m == 2, 1]
        if not bool((one == 0x3F800000).all()):
            out.append(f"{pair}: __expf(0) != 1 or __expf(x <= -128) != 0: 1 / sum of a row with ONE maximal key has bits "
                       f"{sorted({hex(v) for v in one.tolist()})}, not 0x3f800000 (above it: the sum is below 1, so __expf(0) < 1)")
        elif not bool((two == 0x3F000000).all()):
            out.append(f"{pair}: the reciprocal of 2 is not exact: 1 / sum of a row with two maximal keys has bits "
                       f"{sorted({hex(v) for v in two.tolist()})}, not 0x3f000000")
        if not torch.equal(ctx.get(), ref.ctx):
            out.append(f"{pair}: ctx differs from the reference in {int((ctx.get() != ref.ctx).sum())} elements")
    return out


def exact():
    return not precondition_failures()


def test_exp_and_reciprocal_are_exact():
    """the precondition of every torch.equal below.  If this fails, the other tests run their fallback (module docstring)."""
    bad = precondition_failures()
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ the fused kernels
@pytest.mark.parametrize("cs", X.PADDED + X.PADDED_LONG + X.PACKED + X.PACKED_LONG, ids=X.case_id)
def test_fused_attention_exact(cs):
    ref = X.reference(cs)
    run = Launch(cs, ref)
    bits = {pair: run.run(pair, exact()) for pair in cs.pairs}
    if len(bits) == 2:      # (follows from both equalling the reference; stated on its own so that a failure names the pair)
        for a, b, name in zip(bits["res"], bits["long"], ("ctx", "lse", "dqkv")):
            assert torch.equal(a, b), f"{cs.seam}: {name} of {FWD[cs.view, 'res']} / _bwd and of {FWD[cs.view, 'long']} / _bwd differ"


# ------------------------------------------------------------------------------------------------ the unfused path
@pytest.mark.parametrize("T,p,mask,seed", X.SOFTMAX)
def test_unfused_softmax_exact(T, p, mask, seed):
    """mc_softmax_fwd / mc_softmax_bwd on the reference's own score matrices (bias added) and its dP: probs, pd and dS must be
    P, Pd and dS of the reference, with the host Philox mask.  The first SOFTMAX_ROWS rows of the [b nh T, T] matrices."""
    cs = X.softmax_case(T, p, mask, seed)
    ref = X.build(cs, keep_heads=True)
    n = X.SOFTMAX_ROWS
    S, P, Pd, dP, dS = (torch.cat([getattr(h, k) for h in ref.heads])[:n] for k in ("S", "P", "Pd", "dP", "dS"))
    nan = torch.full((64,), float("nan"), dtype=F64)
    scores = torch.cat([S.flatten(), nan]).to(F32).to(DEV)
    assert bool(torch.isfinite(scores[:n * T]).all()) and bool((~(P > 0) | (scores[:n * T].view(n, T).cpu().double() == S)).all())
    dpd = torch.cat([dP.flatten(), nan]).to(F32).to(DEV)
    probs_in = torch.cat([P.flatten(), nan]).to(BF).to(DEV)
    ex = exact()
    for rep in range(2):
        what = f"softmax T {T} p {p} rep {rep}"
        probs, ds = rows_guard(n, T, BF), rows_guard(n, T, BF)
        pd = probs if (p == 0 and rep == 1) else rows_guard(n, T, BF)       # p = 0: also the aliased form ops.softmax_fwd uses
        L.call("mc_softmax_fwd", scores.data_ptr(), n, T, p, X.SEED, X.SID, probs.ptr(), pd.ptr(), ops._st())
        L.call("mc_softmax_bwd", probs_in.data_ptr(), dpd.data_ptr(), n, T, p, X.SEED, X.SID, X.ALPHA, ds.ptr(), ops._st())
        torch.cuda.synchronize()
        for g, name in ((probs, "probs"), (pd, "probs_drop"), (ds, "dscores")):
            g.check(f"{what} {name}")
        same(probs.get(), P, f"{what} probs", ex)
        same(pd.get(), Pd, f"{what} probs_drop", ex)
        same(ds.get(), dS, f"{what} dscores", True)     # (its inputs are the reference's P and dP: nothing inexact enters)
