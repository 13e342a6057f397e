"""Deterministic mode on the device: the store-and-sum endings of the backward scatter-adds (depthwise weight gradients,
LayerNorm gamma / beta, the embedding tables) against the workspace they leave, against themselves over repeated launches,
against fp64 torch references and against the default (atomic) endings.  GPU only (`pytest -m gpu`).
The fp32 bound 1e-4 * max|ref| is DESIGN.md section 3's bound for fp32 kernel outputs."""
import ctypes as C

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
F32 = torch.float32
TOL = 1e-4


def rnd(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def host_sum(ws):
    """float32(sum_r float64(ws[r])), r ascending, one accumulator"""
    acc = torch.zeros(ws.shape[1:], dtype=torch.float64, device=ws.device)
    for r in range(ws.shape[0]):
        acc = acc + ws[r].double()
    return acc.float()


def close(got, ref, what):
    err = float((got.double() - ref.double()).abs().max())
    bound = TOL * float(ref.double().abs().max())
    print(what, "max err", err, "bound", bound)
    assert err <= bound, (what, err, bound)


@pytest.fixture
def lane_mode():
    lib = L.load()
    old = lib.mc_dwconv_set_lane_mode(-1)
    yield lib.mc_dwconv_set_lane_mode
    lib.mc_dwconv_set_lane_mode(old)


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


def with_ws(a, rows_fn, det):
    """arms the argument block with a NaN-filled workspace (every element must be written by the launch)"""
    if not det:
        return None
    rows = getattr(L.load(), rows_fn)(C.byref(a))
    assert rows >= 2, f"{rows_fn}: the shape gives {rows} workspace row(s); the test needs at least 2 per destination"
    ws = torch.full((rows, a.k * a.k, a.c), float("nan"), dtype=F32, device=DEV)
    a.dw_partials, a.dw_rows = ws.data_ptr(), rows
    return ws


def dw_ref64(a_in, g, n, h, w, oh, ow, c, k, stride, pad_l, pad_t):
    """dW[kh*k+kw, c] = sum g[o, j] * a_in[o*s - pt + kh, j*s - pl + kw] in fp64"""
    x = a_in.double().view(n, h, w, c)
    xp = torch.zeros((n, h + 2 * k, w + 2 * k, c), dtype=torch.float64, device=DEV)
    xp[:, pad_t:pad_t + h, pad_l:pad_l + w] = x
    gg = g.double().view(n, oh, ow, c)
    return torch.stack([(gg * xp[:, kh:kh + (oh - 1) * stride + 1:stride, kw:kw + (ow - 1) * stride + 1:stride]).sum((0, 1, 2))
                        for kh in range(k) for kw in range(k)])


def common_checks(run, ref64, what, shape=None):
    """run(det, prefill) -> (dw, ws, extras).  Checks (a)-(d) of the issue and returns the extras of both modes for (e)."""
    shape = tuple(ref64.shape) if shape is None else shape
    zero = lambda: torch.zeros(shape, dtype=F32, device=DEV)      # noqa: E731
    dw_def, _, ex_def = run(False, zero())
    outs = [run(True, zero()) for _ in range(3)]
    torch.cuda.synchronize()
    dw, ws, ex = outs[0]
    assert torch.isfinite(ws).all(), what + ": a workspace element was not written"
    assert torch.equal(dw, host_sum(ws)), what + ": dw is not the ordered fp64 sum of the workspace rows"          # (a)
    for o in outs[1:]:
        assert torch.equal(o[0], dw), what + ": repeated launches differ"                                          # (b)
    if ref64 is not None:
        close(dw, ref64, what + " vs fp64")                                                                       # (c)
    close(dw, dw_def, what + " vs the default mode")
    pre = rnd(*dw.shape, seed=99, dtype=F32)
    dw2, ws2, _ = run(True, pre.clone())
    torch.cuda.synchronize()
    assert torch.equal(dw2, pre + host_sum(ws2)), what + ": a pre-filled dw is not added to"                        # (d)
    for a, b in zip(ex, ex_def):
        assert torch.equal(a, b), what + ": dZ0 / stat_partials differ from the default mode"                      # (e)


BWW_CASES = [(2, 70, 300, 48, 3), (3, 33, 59, 24, 3), (33, 48, 29, 64, 3), (9, 7, 9, 24, 3), (2, 40, 33, 240, 5)]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("n,h,w,c,k", BWW_CASES)
def test_weight_gradient_store_and_sum(lane_mode, mode, n, h, w, c, k):
    """mc_dwconv_bwd_weight with dw_partials: the lane = column BWW ending (mode 1) and the marching bww kernel (mode 0)"""
    lane_mode(mode)
    pad = k // 2
    x, dy = rnd(n * h * w, c, seed=1), rnd(n * h * w, c, seed=2)
    ref = dw_ref64(x, dy, n, h, w, h, w, c, k, 1, pad, pad)

    def run(det, dw):
        a = ops._dw_args(n, h, w, c, k, 1, pad, pad, h, w)
        a.x, a.dy, a.out = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
        ws = with_ws(a, "mc_dwconv_bwd_weight_dw_rows", det)
        L.call("mc_dwconv_bwd_weight", C.byref(a), ops._st())
        return dw, ws, ()
    common_checks(run, ref, f"bww mode {mode} {(n, h, w, c, k)}")
    # (f) a wrong row count is refused before any launch
    a = ops._dw_args(n, h, w, c, k, 1, pad, pad, h, w)
    dw = torch.zeros((k * k, c), dtype=F32, device=DEV)
    a.x, a.dy, a.out = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
    ws = with_ws(a, "mc_dwconv_bwd_weight_dw_rows", True)
    a.dw_rows += 1
    assert L.load().mc_dwconv_bwd_weight(C.byref(a), ops._st()) != 0 and b"dw_partials" in L.load().mc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(ws).all() and not dw.any()


@pytest.mark.parametrize("n,h,w,c", [(2, 70, 300, 48), (3, 33, 59, 24), (33, 48, 29, 64), (9, 7, 9, 24)])
def test_fused_backward_store_and_sum(lane_mode, n, h, w, c):
    """mc_dwconv_bwd_fused (lane FUSED ending) with dw_partials; the fp64 reference takes a0 = silu(bn0(e)) of the stored e"""
    lane_mode(1)
    k, pad = 3, 1
    e, dd = rnd(n * h * w, c, seed=1), rnd(n * h * w, c, seed=2)
    wk = rnd(k * k, c, seed=3, dtype=F32)
    st = bn_stats(e, c, n * h * w, 4)
    wflip = wk.flip(0).contiguous()
    z = e.double() * st.scale.double() + st.shift.double()
    ref = dw_ref64(z * torch.sigmoid(z), dd, n, h, w, h, w, c, k, 1, pad, pad)

    def run(det, dw):
        a = ops._dw_fused_args(dd, wflip, n, h, w, c, k, pad, pad, h, w, e, st)
        dz = torch.empty((n * h * w, c), dtype=BF, device=DEV)
        rows = L.load().mc_dwconv_bwd_fused_stat_rows(C.byref(a))
        part = torch.empty((rows, 2, c), dtype=F32, device=DEV)
        a.out, a.dw_out, a.stat_partials, a.stat_rows = dz.data_ptr(), dw.data_ptr(), part.data_ptr(), rows
        ws = with_ws(a, "mc_dwconv_bwd_fused_dw_rows", det)
        L.call("mc_dwconv_bwd_fused", C.byref(a), ops._st())
        return dw, ws, (dz, part)
    common_checks(run, ref, f"fused {(n, h, w, c)}")
    a = ops._dw_fused_args(dd, wflip, n, h, w, c, k, pad, pad, h, w, e, st)
    dw = torch.zeros((k * k, c), dtype=F32, device=DEV)
    dz = torch.empty((n * h * w, c), dtype=BF, device=DEV)
    rows = L.load().mc_dwconv_bwd_fused_stat_rows(C.byref(a))
    part = torch.empty((rows, 2, c), dtype=F32, device=DEV)
    a.out, a.dw_out, a.stat_partials, a.stat_rows = dz.data_ptr(), dw.data_ptr(), part.data_ptr(), rows
    with_ws(a, "mc_dwconv_bwd_fused_dw_rows", True)
    a.dw_rows += 1
    assert L.load().mc_dwconv_bwd_fused(C.byref(a), ops._st()) != 0 and b"dw_partials" in L.load().mc_last_error()


def test_stride2_data_gradient_store_and_sum(lane_mode):
    """mc_dwconv_bwd_data with xw + dw_out + dw_partials, case (5, 38, 22, 64, 384, (0, 1)) of tests/test_dw_s2_efree_gpu.py.
    The fp64 reference: e = the 16-bit tensor the expand GEMM stores (ops.linear_fwd, what the launch forms on the MFMA unit),
    a0 = silu(bn0(e)) rounded to the storage type as the staging does, dW[kh, kw, c] = sum dd[o, j] * a0[2o - pt + kh, 2j - pl + kw]."""
    lane_mode(0)
    n, h, w, cin, c, pad = 5, 38, 22, 64, 384, (0, 1)
    oh, ow = (h + 1) // 2, (w + 1) // 2
    x, we = rnd(n * h * w, cin, seed=71), rnd(c, cin, seed=72, scale=cin ** -0.5)
    dd, wk = rnd(n * oh * ow, c, seed=73), rnd(9, c, seed=74, dtype=F32)
    e = ops.linear_fwd(x, we)
    st = bn_stats(e, c, n * h * w, 75)
    a0 = torch.nn.functional.silu(torch.addcmul(st.shift, e.float(), st.scale)).to(BF)
    ref = dw_ref64(a0, dd, n, h, w, oh, ow, c, 3, 2, pad[0], pad[1])

    def args(dw):
        a = ops._dw_args(n, h, w, c, 3, 2, pad[0], pad[1], oh, ow)
        dz = torch.empty((n * h * w, c), dtype=BF, device=DEV)
        a.dy, a.out, a.w_kkc = dd.data_ptr(), dz.data_ptr(), wk.data_ptr()
        a.epi_x, a.epi_scale, a.epi_shift, a.epi_mean, a.epi_invstd = (x.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(),
                                                                       st.mean.data_ptr(), st.invstd.data_ptr())
        a.xw, a.cin = we.data_ptr(), cin
        rows = L.load().mc_dwconv_bwd_data_stat_rows(C.byref(a))
        part = torch.empty((rows, 2, c), dtype=F32, device=DEV)
        a.stat_partials, a.stat_rows, a.dw_out = part.data_ptr(), rows, dw.data_ptr()
        return a, dz, part

    def run(det, dw):
        a, dz, part = args(dw)
        ws = with_ws(a, "mc_dwconv_bwd_data_dw_rows", det)
        L.call("mc_dwconv_bwd_data", C.byref(a), ops._st())
        return dw, ws, (dz, part)
    common_checks(run, ref, "stride-2 xw + dw_out")
    a, _, _ = args(torch.zeros((9, c), dtype=F32, device=DEV))
    with_ws(a, "mc_dwconv_bwd_data_dw_rows", True)
    a.dw_rows += 1
    assert L.load().mc_dwconv_bwd_data(C.byref(a), ops._st()) != 0 and b"dw_partials" in L.load().mc_last_error()


def test_ordered_sum_entry_point():
    ws = rnd(37, 1000, seed=5, dtype=F32) * 1e3
    out = rnd(1000, seed=6, dtype=F32)
    pre = out.clone()
    L.call("mc_ordered_sum", ws.data_ptr(), 37, 1000, 1000, out.data_ptr(), 1, ops._st())
    assert torch.equal(out, pre + host_sum(ws))
    L.call("mc_ordered_sum", ws.data_ptr(), 37, 1000, 333, out.data_ptr(), 0, ops._st())
    assert torch.equal(out[:333], host_sum(ws)[:333]) and torch.equal(out[333:], (pre + host_sum(ws))[333:])


GRIDCAP = 512     # workgroups of add_ln_bwd_k at most (mc_add_ln_bwd_ws_rows)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rows", [4 * GRIDCAP + 3, 5])
@pytest.mark.parametrize("h", [768, 256])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_add_ln_bwd_store_and_sum(packed, rows, h, p):
    lib = L.load()
    wr = lib.mc_add_ln_bwd_ws_rows(rows)
    assert wr >= 2 and (rows < 4 * GRIDCAP or wr == GRIDCAP)
    dy, x, res = rnd(rows, h, seed=1), rnd(rows, h, seed=2), rnd(rows, h, seed=3)
    gamma = rnd(h, seed=4, dtype=F32) * 0.2 + 1.0
    row_map = None
    if packed:
        row_map = torch.arange(rows, dtype=torch.int32, device=DEV) * 2        # every packed row maps to another padded row
        row_map[-1] = -1                                                       # ... and one alignment row
    # the dropout factors of (seed 1234, stream 7): mc_dropout_f32 draws them by the same (seed, stream id, element / 8) rule, the
    # element index formed from the row of the padded layout; alignment rows are not dropped
    ds = torch.ones(rows, h, dtype=F32, device=DEV)
    if p > 0.0:
        drows = rows if row_map is None else 2 * rows
        ds = ops.dropout_f32(torch.ones(drows * h, dtype=F32, device=DEV), p, 1234, 7).view(drows, h)
        if row_map is not None:
            ds = ds[row_map.clamp(min=0).long()]
            ds[row_map < 0] = 1.0
        assert 0.05 < float((ds == 0).float().mean()) < 0.15
    s = x.float() * ds + res.float()
    mean, rstd = s.mean(1).contiguous(), (s.var(1, unbiased=False) + 1e-12).rsqrt().contiguous()
    rm = () if row_map is None else (row_map.data_ptr(),)
    name = "mc_add_ln_bwd" if row_map is None else "mc_add_ln_rows_bwd"

    def run(det, gb):
        dx, dres = torch.empty_like(x), torch.empty_like(x)
        ws, wsa = None, ()
        if det:
            ws = torch.full((wr, 2, h), float("nan"), dtype=F32, device=DEV)
            wsa = (ws.data_ptr(), wr)
        L.call(name + ("_ws" if det else ""), dy.data_ptr(), x.data_ptr(), res.data_ptr(), *rm, gamma.data_ptr(), mean.data_ptr(),
               rstd.data_ptr(), rows, h, p, 1234, 7, dx.data_ptr(), dres.data_ptr(), gb[0].data_ptr(), gb[1].data_ptr(), *wsa, ops._st())
        return gb, ws, (dx, dres)
    xh = (x.double() * ds.double() + res.double() - mean.double()[:, None]) * rstd.double()[:, None]
    ref = torch.stack([(dy.double() * xh).sum(0), dy.double().sum(0)])
    common_checks(run, ref, f"add_ln_bwd packed={packed} rows={rows} h={h} p={p}", shape=(2, h))
    gb = torch.zeros((2, h), dtype=F32, device=DEV)
    dx = torch.empty_like(x)
    ws = torch.empty((wr + 1, 2, h), dtype=F32, device=DEV)
    st = getattr(lib, name + "_ws")(dy.data_ptr(), x.data_ptr(), res.data_ptr(), *rm, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                    rows, h, p, 1234, 7, dx.data_ptr(), dx.data_ptr(), gb[0].data_ptr(), gb[1].data_ptr(), ws.data_ptr(),
                                    wr + 1, ops._st())
    assert st != 0 and b"ws_rows" in lib.mc_last_error()


@pytest.mark.parametrize("packed", [False, True])
def test_bert_embed_bwd_store_and_sum(packed):
    h, vocab, b, t = 768, 50, 3, 17
    lengths = [17, 1, 9] if packed else [t] * b
    g = torch.Generator().manual_seed(3)
    ids2 = torch.randint(10, 30, (b, t), generator=g)
    ids2[torch.rand(b, t, generator=g) < 0.6] = 0                     # id 0 in more than half of the rows; ids 30 .. 49 never occur
    ids2[0, 0] = 0
    tt2 = (torch.arange(t)[None, :] >= 8).long().expand(b, t).contiguous()
    word, pos, typ = rnd(vocab, h, seed=1, dtype=F32), rnd(64, h, seed=2, dtype=F32), rnd(2, h, seed=3, dtype=F32)
    gamma = rnd(h, seed=4, dtype=F32) * 0.2 + 1.0
    beta = rnd(h, seed=5, dtype=F32) * 0.1
    pk = None
    if packed:
        pk = ops.PackedRows(lengths, t).to(DEV)
        ids = torch.index_select(ids2.reshape(-1).to(DEV), 0, pk.src.long())
        tt = torch.index_select(tt2.reshape(-1).to(DEV), 0, pk.src.long())
        real = pk.real
    else:
        ids, tt, real = ids2.to(DEV), tt2.to(DEV), b * t
    flat_ids = ids.reshape(-1)[:real]
    assert int((flat_ids == 0).sum()) * 2 > real and len(set(flat_ids.tolist())) < vocab and set(tt.reshape(-1)[:real].tolist()) == {0, 1}
    y, mean, rstd = ops.bert_embed_fwd(ids, tt, word, pos, typ, gamma, beta, 1e-12, 0.0, 11, 3, pk=pk)
    rows_out = y.shape[0]
    dy = rnd(rows_out, h, seed=6)
    plan = (C.c_int * 2)()
    tmax = max(lengths)
    nfl = L.load().mc_bert_embed_bwd_ws_floats(b, tmax, h, real, plan)
    assert plan[0] >= 2 and plan[1] >= 2, "at least 2 workspace rows per destination"
    sorted_ids, order = ops.token_rows_by_id(flat_ids)
    pre = [rnd(*s, seed=20 + i, dtype=F32) for i, s in enumerate([(vocab, h), (64, h), (2, h), (h,), (h,)])]

    def run():
        outs = [q.clone() for q in pre]
        ws = torch.full((nfl,), float("nan"), dtype=F32, device=DEV)
        tail = (0.0, 11, 3, *[o.data_ptr() for o in outs], sorted_ids.data_ptr(), order.data_ptr(), ws.data_ptr(), nfl, ops._st())
        if pk is None:
            L.call("mc_bert_embed_bwd_ws", dy.data_ptr(), ids.data_ptr(), tt.data_ptr(), word.data_ptr(), pos.data_ptr(), typ.data_ptr(),
                   gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), b, t, h, *tail)
        else:
            L.call("mc_bert_embed_rows_bwd_ws", dy.data_ptr(), ids.data_ptr(), tt.data_ptr(), pk.cu.data_ptr(), word.data_ptr(),
                   pos.data_ptr(), typ.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), pk.b, pk.max_len, pk.t, h, real,
                   *tail)
        return outs, ws
    runs = [run() for _ in range(3)]
    torch.cuda.synchronize()
    outs, ws = runs[0]
    assert torch.isfinite(ws).all(), "a workspace element was not written"
    for o2, _ in runs[1:]:
        assert all(torch.equal(a, c) for a, c in zip(outs, o2)), "repeated launches differ"
    dword, dpos, dtyp, dgamma, dbeta = [o - q for o, q in zip(outs, pre)]
    # vocabulary rows that no token names keep their pre-fill, bit for bit
    unused = torch.ones(vocab, dtype=torch.bool, device=DEV)
    unused[flat_ids] = False
    assert unused.any() and torch.equal(outs[0][unused], pre[0][unused])
    # dword rows = the stored per-row dx summed in ascending row order
    dxrows = ws[:real * h].view(real, h)
    for i in sorted(set(flat_ids.tolist())):
        rows_i = (flat_ids == i).nonzero().flatten().tolist()
        assert rows_i == sorted(rows_i)
        assert torch.equal(outs[0][i], pre[0][i] + host_sum(dxrows[rows_i])), f"dword row {i}"
    # fp64 index_add_ reference (dx from the same formulas in fp64, from the kernel's own inputs)
    tp = (pk.pos[:real] if packed else torch.arange(t, device=DEV).repeat(b)).long()
    tf = tt.reshape(-1)[:real]
    emb = word.double()[flat_ids] + pos.double()[tp] + typ.double()[tf]
    xh = (emb - mean.double()[:real, None]) * rstd.double()[:real, None]
    d = dy.double()[:real]
    dg = d * gamma.double()
    dx = rstd.double()[:real, None] * (dg - dg.mean(1, keepdim=True) - xh * (dg * xh).mean(1, keepdim=True))
    close(dxrows, dx, "dx rows")
    refs = [torch.zeros(vocab, h, dtype=torch.float64, device=DEV).index_add_(0, flat_ids, dx),
            torch.zeros(64, h, dtype=torch.float64, device=DEV).index_add_(0, tp, dx),
            torch.zeros(2, h, dtype=torch.float64, device=DEV).index_add_(0, tf, dx), (d * xh).sum(0), d.sum(0)]
    for name, got, ref in zip(("dword", "dpos", "dtype", "dgamma", "dbeta"), (dword, dpos, dtyp, dgamma, dbeta), refs):
        # (got = out - prefill carries the rounding of the += onto a prefill of unit scale: half an ulp of max|out|)
        err, bound = float((got.double() - ref).abs().max()), TOL * float(ref.abs().max())
        print(name, err, bound)
        assert err <= bound, (name, err, bound)


def test_ops_wrappers_follow_the_switch():
    """ops.add_ln_bwd / bert_embed_bwd (padded and packed) / dwconv_bwd_weight under set_deterministic(True): same bits on every call"""
    prev = ops.set_deterministic(True)
    try:
        rows, h = 301, 768
        dy, x, res = rnd(rows, h, seed=1), rnd(rows, h, seed=2), rnd(rows, h, seed=3)
        gamma = rnd(h, seed=4, dtype=F32)
        mean, rstd = rnd(rows, seed=5, dtype=F32), rnd(rows, seed=6, dtype=F32).abs() + 0.5
        a = [ops.add_ln_bwd(dy, x, res, gamma, mean, rstd, 0.1, 5, 2) for _ in range(3)]
        n, hh, w, c = 3, 33, 59, 24
        xx, dd = rnd(n * hh * w, c, seed=7), rnd(n * hh * w, c, seed=8)
        d = [ops.dwconv_bwd_weight(xx, dd, n, hh, w, c, 3, 1, 1, 1, hh, w) for _ in range(3)]
        word, pos, typ = rnd(50, h, seed=9, dtype=F32), rnd(32, h, seed=10, dtype=F32), rnd(2, h, seed=11, dtype=F32)
        ids2 = (torch.arange(3 * 17).view(3, 17) % 7).to(DEV)
        tt2 = (ids2 % 2).contiguous()
        emb = []
        for pk in (None, ops.PackedRows([17, 1, 9], 17).to(DEV)):
            ids = ids2 if pk is None else torch.index_select(ids2.reshape(-1), 0, pk.src.long())
            tt = tt2 if pk is None else torch.index_select(tt2.reshape(-1), 0, pk.src.long())
            y, m, rs = ops.bert_embed_fwd(ids, tt, word, pos, typ, gamma, gamma, 1e-12, 0.1, 11, 3, pk=pk)
            dye = rnd(y.shape[0], h, seed=12)
            emb.append([ops.bert_embed_bwd(dye, ids, tt, word, pos, typ, gamma, m, rs, 0.1, 11, 3, pk=pk) for _ in range(3)])
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for r in a[1:] for u, v in zip(a[0], r))
        assert torch.equal(d[0], d[1]) and torch.equal(d[0], d[2])
        for runs in emb:
            assert all(torch.isfinite(u).all() and torch.equal(u, v) for r in runs[1:] for u, v in zip(runs[0], r))
    finally:
        assert ops.set_deterministic(prev) is True
    assert ops.deterministic() == prev


def _build_step(packed_text):
    import types
    from mammo_clip_amd import engine
    from mammo_clip_amd.breastclip import util
    from mammo_clip_amd.breastclip.loss import build_loss
    from mammo_clip_amd.breastclip.model import build_model
    from mammo_clip_amd.breastclip.optimizer import build_optimizer
    from oracle import arch as oarch, bert as obert, weights as ow
    cfg = {"name": "clip_custom", "temperature": 0.07,
           "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
           "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                            "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
           "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
    loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
    sd = ow.synth_state_dict(ow.clip_shapes(oarch.build_arch("efficientnet-b2"), obert.BertShape()), seed=10)
    batch = ow.synth_batch(4, 224, 224, 64, seed=3)
    if packed_text:                                               # the opt-in packed text encoder (config key text_encoder.packed)
        cfg["text_encoder"]["packed"] = True
    bt = {"images": batch["images"].to(DEV), "image_views": batch["image_views"].to(DEV),
          "text_tokens": {k: v.to(DEV) for k, v in batch["text_tokens"].items()},
          "text_tokens2": {k: v.to(DEV) for k, v in batch["text_tokens2"].items()}}

    def one(**step_kw):
        util.GlobalEnv.reset()
        torch.manual_seed(1234)
        model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996))
        model.load_state_dict(sd, strict=True)
        model = model.to(DEV)
        assert model.text_encoder.packed == packed_text
        if packed_text:                                           # the call really runs packed: add_ln_bwd with a row_map and
            with torch.no_grad():                                 # mc_bert_embed_rows_bwd_ws are then on the step's path
                assert model.text_encoder.forward_packed(bt["text_tokens"])[1] is not None
        opt = build_optimizer(model, {"name": "adamw", "config": {"lr": 5e-5, "weight_decay": 1e-4}})
        tr = engine.Trainer(model, build_loss(loss_cfg), opt, None, DEV, deterministic=True, **step_kw.pop("trainer", {}))
        ld = tr.step(bt, **step_kw)
        torch.cuda.synchronize()
        assert ops.deterministic() is False
        params = {n: p.detach().clone() for n, p in model.named_parameters()}
        avg = {n: opt.state[p]["exp_avg"].clone() for n, p in model.named_parameters() if p in opt.state and "exp_avg" in opt.state[p]}
        return params, avg, {k: v.detach().clone() for k, v in ld.items() if torch.is_tensor(v)}
    return one


@pytest.mark.parametrize("variant", ["single", "micro", "packed"])
def test_whole_step_is_bit_reproducible(variant):
    """two Trainer(deterministic=True).step() calls from the same state, batch and seed: every parameter, every exp_avg and the
    loss dict bit-equal (config #1: B2, 224 x 224, T = 64, 4 pairs, two views and two reports)"""
    one = _build_step(variant == "packed")
    kw = dict(micro_batches=2, trainer=dict(keep_graphs=1)) if variant == "micro" else {}
    p1, a1, l1 = one(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in kw.items()})
    p2, a2, l2 = one(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in kw.items()})
    assert len(a1) > 0 and a1.keys() == a2.keys()
    diff = [n for n in p1 if not torch.equal(p1[n], p2[n])] + ["exp_avg:" + n for n in a1 if not torch.equal(a1[n], a2[n])]
    assert not diff, (len(diff), diff[:8])
    assert l1.keys() == l2.keys() and all(torch.equal(l1[k], l2[k]) for k in l1), "loss dict"


def test_mode_is_restored_after_a_step_that_raises():
    from mammo_clip_amd import engine

    m = torch.nn.Linear(1, 1).to(DEV)
    tr = engine.Trainer(m, None, torch.optim.SGD(m.parameters(), lr=0.0), None, DEV, deterministic=True)

    def boom(batch):
        assert ops.deterministic() is True
        raise RuntimeError("boom")
    tr._step_single = boom
    assert ops.deterministic() is False
    with pytest.raises(RuntimeError, match="boom"):
        tr.step({})
    assert ops.deterministic() is False
