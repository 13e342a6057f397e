"""Every row of the exact-arithmetic attention tables (tests/_attn_exact_cases.py), without a device: the operands build, the
fp64 reference proves the conditions under which the kernels' arithmetic is exact (for bf16 and f16 storage alike), and the
row's numbers reach the block, chunk and sequence seam it names -- so a changed table fails here instead of silently emptying
tests/test_attn_exact_gpu.py.  The host Philox generator behind the dropout masks is checked on its own: the published
known-answer vectors of Philox4x32-10, its keep rate, and its independence of how the elements are grouped into calls."""
import numpy as np
import pytest
import torch

import _attn_exact_cases as X


@pytest.mark.parametrize("cs", X.CASES, ids=X.case_id)
def test_row_builds_exact_and_reaches_its_seam(cs):
    r = X.reference(cs)              # asserts the exactness conditions
    R, H = X.total_rows(cs), cs.nh * X.HD
    assert r.qkv.shape == r.dqkv.shape == (R, 3 * H) and r.dctx.shape == r.ctx.shape == (R, H)
    real = sum(X.seq_lens(cs))
    # operands fit the storage types; alignment rows are NaN on the way in and zero on the way out
    for t in (r.qkv[:real], r.dctx[:real]):
        X.survives(t, cs.seam)
    assert bool(torch.isnan(r.qkv[real:]).all()) and bool(torch.isnan(r.dctx[real:]).all())
    assert not bool(r.ctx[real:].any()) and not bool(r.dqkv[real:].any())
    if cs.view == "packed":
        assert cs.shift and R % 8 == 0 and R - real >= cs.extra and X.t_pad(cs) >= max(cs.lens)
        assert bool(torch.isnan(r.lse[real:]).all()) and bool(torch.isfinite(r.lse[:real]).all())
    else:
        assert cs.t % 32 == 0 and bool(torch.isfinite(r.lse).all())
        live = r.maskb == 0
        assert bool(live.any(1).all()), "a fully masked row is not covered"
        assert bool((~live).any()) == (cs.mask != "none")
    # the row maximum is 256 (-256 with the shift), 1 / row sum a power of two
    fin = r.lse[torch.isfinite(r.lse[..., 0])]
    assert set(fin[:, 0].tolist()) == {-256.0 if cs.shift else 256.0} and set(fin[:, 1].tolist()) <= {1.0, 0.5, 0.25, 0.125}
    if cs is not X.PRECONDITION:
        assert len(set(fin[:, 1].tolist())) >= 3
    # the seams, from the row's numbers
    have = X.seams(cs)
    for name, want in cs.reach:
        assert want <= have[name], (cs.seam, name, sorted(want), sorted(have[name]))
    assert ("res" in cs.pairs) == (max(X.seq_lens(cs)) <= 256) and "long" in cs.pairs
    order = X.order_of(cs)
    assert order is None or sorted(order.tolist()) == list(range(cs.b))


def test_tables_cover_every_seam_of_the_issue():
    """sizes, masks, dropout rates, orders and alignment rows per view and kernel pair"""
    def rows(table, **kw):
        return [c for c in table if all(getattr(c, k) == v for k, v in kw.items())]
    for t in (32, 64, 160, 256):
        assert {c.mask for c in rows(X.PADDED, t=t)} == {"none", "length", "holes"}
        assert {c.p for c in rows(X.PADDED, t=t)} == {0.0, 0.5}
    assert rows(X.PADDED, shift=True) and rows(X.PADDED_LONG, shift=True)
    assert {c.t for c in X.PADDED_LONG} == {32, 256, 288, 384, 512}
    assert {c.p for c in X.PADDED_LONG} == {0.0, 0.5, 0.75}
    for c in rows(X.PADDED_LONG, mask="holes"):
        if c.t > 256:
            dead = (~X.live_keys(c, 0)).nonzero().flatten()
            assert bool((dead < 256).any()) and bool((dead >= 256).any()) and 255 in dead and 256 in dead
    assert [c for c in rows(X.PADDED_LONG, mask="holes") if c.t > 256]
    holes = ~X.live_keys(rows(X.PADDED, t=64, mask="holes")[0], 0)
    assert bool(holes[0]) and bool(holes[31]) and bool(holes[32]) and bool(holes[-7:].any()) and not bool(holes[-7:].all())
    assert {c.lens for c in X.PACKED} == {X.LENS_A, X.LENS_B}
    assert X.LENS_A == (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256) and X.LENS_B == (33, 1, 256, 64)
    assert {c.lens for c in X.PACKED_LONG} >= {(257, 1, 511, 33, 512, 256, 289, 300), (512,), (257,)}
    for table in (X.PACKED, X.PACKED_LONG):
        assert {c.order for c in table} == {None, "longest", "scrambled"} and {c.p for c in table} == {0.0, 0.5}
        assert any(X.total_rows(c) > sum(c.lens) for c in table), "no row with alignment rows"
        assert any(c.t % 8 for c in table) and any(X.t_pad(c) // 8 % 4 for c in table)
        assert {c.nh for c in table} == {1, 3}
    assert {c.t for c in X.PACKED_LONG} == {512, 300} and X.t_pad(rows(X.PACKED_LONG, t=300)[0]) == 304
    for c in X.CASES:
        assert c.nh in (1, 3) and 1 <= c.b <= 12 and (c.view == "packed" or c.b in (2, 3))
    scr = [X.order_of(c).tolist() for c in X.CASES if c.order == "scrambled"]
    lng = [X.order_of(c).tolist() for c in X.CASES if c.order == "longest"]
    assert all(o != sorted(o) for o in scr) and all(o != sorted(o) for o in lng)
    # the unfused path: the general form and the three widths of the 8-keys-per-lane form, each with and without dropout
    assert {t for t, _, _, _ in X.SOFTMAX} == {40, 100, 64, 256, 512}
    for t in (40, 64, 256, 512):
        assert {p for tt, p, _, _ in X.SOFTMAX if tt == t} == {0.0, 0.5}
    for t, p, _, _ in X.SOFTMAX:
        g = t // 8
        assert (t in (64, 256, 512)) == (t % 8 == 0 and 2 <= g <= 64 and g & (g - 1) == 0) and (p == 0 or t % 8 == 0)


@pytest.mark.parametrize("T,p,mask,seed", X.SOFTMAX)
def test_unfused_rows_build(T, p, mask, seed):
    cs = X.softmax_case(T, p, mask, seed)
    r = X.build(cs, keep_heads=True)
    assert len(r.heads) == cs.b * cs.nh and r.heads[0].S.shape == (T, T)
    assert cs.b * cs.nh * T > X.SOFTMAX_ROWS
    # the scores with the bias added are the same numbers in fp32
    S = torch.cat([h.S for h in r.heads])
    assert bool(torch.isfinite(S.float()).all()) and bool(((S.float().double() == S) | (S < -1e38)).all())


def test_philox_known_answers():
    """the three known-answer vectors of Philox4x32-10 (Random123, kat_vectors)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = X.philox4x32_10(*(np.array([c], dtype=np.uint64) for c in ctr), *key)
        assert tuple(int(w[0]) for w in got) == want


def test_philox_keep_rate_and_thresholds():
    """a property of the generator, not of a kernel: at p = 0.5 the keep rate over 2^17 elements lies in [0.49, 0.51]"""
    keep = X.keep8(X.SEED, X.SID, np.arange(1 << 14), 0.5)
    assert keep.shape == (1 << 14, 8) and keep.size >= 1 << 16
    assert 0.49 <= keep.mean() <= 0.51
    for j in range(8):                     # every one of the eight halves on its own
        assert 0.47 <= keep[:, j].mean() <= 0.53
    k75 = X.keep8(X.SEED, X.SID, np.arange(1 << 14), 0.75)
    assert 0.24 <= k75.mean() <= 0.26 and not bool((k75 & ~keep).any())       # a higher threshold keeps a subset
    assert bool(X.keep8(X.SEED, X.SID, np.arange(64), 0.0).all())
    assert bool((X.keep8(X.SEED, X.SID + 1, np.arange(256), 0.5) != keep[:256]).any())
    assert bool((X.keep8(X.SEED ^ (1 << 40), X.SID, np.arange(256), 0.5) != keep[:256]).any()), "the seed's high word is unused"
    lo, hi = X.keep8(X.SEED, X.SID, np.array([5]), 0.5), X.keep8(X.SEED, X.SID, np.array([5 + (1 << 32)]), 0.5)
    assert bool((lo != hi).any()), "the index's high word is unused"


def test_philox_mask_does_not_depend_on_the_grouping():
    """the mask of an element is a function of (seed, stream, element): whole matrix, row by row, key block by key block"""
    T, bh, p = 304, 5, 0.5
    whole = X.keep_matrix(bh, T, 257, 257, p)
    assert whole.shape == (257, 257) and set(whole.unique().tolist()) == {0.0, 2.0}
    for q in (0, 100, 256):
        row = X.keep8(X.SEED, X.SID, (bh * T + q) * (T // 8) + np.arange(33), p).reshape(-1)[:257]
        assert torch.equal(torch.from_numpy(row).double() * 2, whole[q])
    idx = np.random.default_rng(0).permutation(257 * 38)[:4096]      # single groups in a scrambled order
    q, k8 = idx // 38, idx % 38
    one = X.keep8(X.SEED, X.SID, (bh * T + q) * (T // 8) + k8, p)
    for j in (0, 3, 7):
        ok = k8 * 8 + j < 257
        assert torch.equal(torch.from_numpy(one[ok, j]).double() * 2, whole[q[ok], (k8 * 8 + j)[ok]])
    # a sequence of a packed batch draws the top-left corner of its padded matrix
    assert torch.equal(X.keep_matrix(bh, T, 33, 33, p), whole[:33, :33])
    assert torch.equal(X.keep_matrix(bh, T, 8, 8, 0.75) != 0, (X.keep_matrix(bh, T, 8, 8, 0.75) == 4.0))
