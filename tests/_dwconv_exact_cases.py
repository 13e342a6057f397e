"""Case tables and fp64 references of the exact-arithmetic depthwise tests (test_dwconv_exact_routes.py on the CPU,
test_dwconv_exact_gpu.py on the device).  Nothing here needs a GPU.

Exactness.  Plain cases: x and dy from {-1, +1}, taps from {+-1, +-2, +-3}: every output is an integer of magnitude <= 75 (the
16-bit storage type holds it), every fp32 partial sum is an exact integer whatever the order, so the comparison with the fp64
conv2d / autograd reference is torch.equal.  Saturated cases (sat): BatchNorm scale 1, shift 19 on e in {-1, +1} gives z in {18, 20},
where sigmoid_f (common_hip.h) is exactly 1: the prologue forms a0 = e + 19, silu' is 1, so the epilogue leaves dZ0 = dA0, the
BatchNorm-backward partials (mean 0, invstd 1) are sum dZ0 and sum dZ0 * e, and the fused dW = sum dd * a0 -- all exact integers.
A prologue forward yields even integers (representable to 512): its taps come from {+-1} (5x5, |y| <= 500) or {+-1, +-2} (3x3,
|y| <= 360).  check_exact() asserts these conditions on the reference itself.

A case is (kind, lane, k, s, n, h, w, c, sat, seam, want): (h, w) is the conv's INPUT map, lane the forced lane mode (0 marching,
1 lane = column), `seam` names what the row is there for and `want` what the library's plan queries must answer for it.
kinds: fwd (forward + statistics; sat: with the prologue), wgrad (weight gradient; sat: prologue), gather (stride-1 gather data
gradient), dgrad2 (stride-2 data gradient; sat: BatchNorm-backward epilogue), dgrad1 (stride-1 data gradient on flipped taps with
the epilogue), fused (the whole stride-1 backward in one launch)."""
import collections
import ctypes as C
import functools

import torch
import torch.nn.functional as F

from mammo_clip_amd import lib as L

ST = torch.bfloat16 if L.STORAGE == "bf16" else torch.float16        # the 16-bit storage dtype (= ops.BF16)
TWO24 = 1 << 24
SHIFT = 19.0                                                          # z = e + 19 in {18, 20}

Case = collections.namedtuple("Case", "kind lane k s n h w c sat seam want")


def same_pad(size, k, s):
    """static "same" padding: (pad in front, output size); the rest of the padding lies behind (asymmetric for stride 2)"""
    out = -(-size // s)
    return max((out - 1) * s + k - size, 0) // 2, out


def geom(cs):
    pt, oh = same_pad(cs.h, cs.k, cs.s)
    pl, ow = same_pad(cs.w, cs.k, cs.s)
    return pl, pt, oh, ow


def case_id(cs):
    return f"{cs.kind}{'-sat' if cs.sat else ''}-{'lane' if cs.lane else 'march'}-k{cs.k}s{cs.s}-{cs.n}x{cs.h}x{cs.w}x{cs.c}-{cs.seam}"


# ------------------------------------------------------------------------------------------------------------ references
Ref = collections.namedtuple("Ref", "e dy wk y dx dw")


@functools.lru_cache(maxsize=2)
def reference(k, s, n, h, w, c, sat):
    """fp64 conv2d + autograd on the integers, NHWC: e [n,h,w,c] (the stored input), dy [n,oh,ow,c], wk [k*k,c] (the conv's own
    tap order), y = conv(a0), dx = dL/da0, dw = dL/dwk with a0 = e (+ 19 where sat).  Treat the result as read-only."""
    g = torch.Generator().manual_seed(((k * 3 + s) * 7919 + n * 104729 + h * 1299709 + w * 15485863 + c) % (1 << 31) + int(sat))
    pt, oh = same_pad(h, k, s)
    pl, ow = same_pad(w, k, s)
    pm = lambda *shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()
    e, dy = pm(n, h, w, c), pm(n, oh, ow, c)
    mags = torch.tensor(((1.0,) if k == 5 else (1.0, 2.0)) if sat else (1.0, 2.0, 3.0), dtype=torch.float64)
    wk = mags[torch.randint(0, len(mags), (k * k, c), generator=g)] * pm(k * k, c)
    a = (e + SHIFT if sat else e).permute(0, 3, 1, 2).clone().requires_grad_(True)
    wt = wk.t().reshape(c, 1, k, k).clone().requires_grad_(True)
    pad = (pl, (ow - 1) * s + k - w - pl, pt, (oh - 1) * s + k - h - pt)
    assert min(pad) >= 0
    y = F.conv2d(F.pad(a, pad), wt, None, s, 0, 1, c)                   # the padding is zero AFTER the activation
    assert y.shape == (n, c, oh, ow)
    dx, dw = torch.autograd.grad(y, (a, wt), dy.permute(0, 3, 1, 2))
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return Ref(e, dy, wk, nhwc(y), nhwc(dx), dw.reshape(c, k * k).t().contiguous())


def ref_of(cs):
    return reference(cs.k, cs.s, cs.n, cs.h, cs.w, cs.c, cs.sat)


# The fallback of the saturated cases, for a device whose sigmoid does not saturate as derived above: Gaussian operands rounded to
# the storage type, a real BatchNorm, an fp64 reference and the bounds of test_kernels_gpu.py instead of equality.
FALLBACK_MAX_PIXELS = 4096      # n * oh * ow: a lost row segment of 8 products then moves a tap gradient by more than 1 %
TOL_OUT, TOL_DW, TOL_PART = 1e-2, 4e-3, 2e-4
GaussRef = collections.namedtuple("GaussRef", "e dy wk scale shift mean invstd y dx_a0 dsilu dw_rounded dw")


@functools.lru_cache(maxsize=2)
def reference_gauss(k, s, n, h, w, c):
    """as reference(), on Gaussian operands with a0 = silu(e * scale + shift): y and dw_rounded from a0 rounded to the storage type
    (what the prologue stages), dw from the unrounded a0 (the fused backward), dx_a0 = dL/da0 and dsilu = silu'(z): dZ0 = dx_a0 * dsilu"""
    g = torch.Generator().manual_seed(k * 1000003 + s * 7919 + n * 104729 + h * 1299709 + w * 15485863 + c)
    pt, oh = same_pad(h, k, s)
    pl, ow = same_pad(w, k, s)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    e, dy = rn(n, h, w, c).to(ST).double(), rn(n, oh, ow, c).to(ST).double()
    wk = (rn(k * k, c) * 0.3).float().double()
    scale, shift = (rn(c) * 0.2 + 1.0).float().double(), (rn(c) * 0.1).float().double()
    mean, invstd = e.mean((0, 1, 2)).float().double(), (e.var((0, 1, 2), unbiased=False) + 1e-3).rsqrt().float().double()
    z = e * scale + shift
    sg = torch.sigmoid(z)
    a0, dsilu = z * sg, sg * (1 + z * (1 - sg))
    pad = (pl, (ow - 1) * s + k - w - pl, pt, (oh - 1) * s + k - h - pt)
    wt = wk.t().reshape(c, 1, k, k).clone().requires_grad_(True)
    out = []
    for act in (a0.to(ST).double(), a0):
        a = act.permute(0, 3, 1, 2).clone().requires_grad_(True)
        y = F.conv2d(F.pad(a, pad), wt, None, s, 0, 1, c)
        dx, dw = torch.autograd.grad(y, (a, wt), dy.permute(0, 3, 1, 2))
        out.append((y.detach().permute(0, 2, 3, 1).contiguous(), dx.permute(0, 2, 3, 1).contiguous(), dw.reshape(c, k * k).t().contiguous()))
    return GaussRef(e, dy, wk, scale, shift, mean, invstd, out[0][0], out[0][1], dsilu, out[0][2], out[1][2])


def survives_storage(t):
    return torch.equal(t.to(ST).double(), t)


def check_exact(cs, r):
    """the conditions under which the kernels' arithmetic is exact, asserted on the reference.  Returns (sums exact, sums of
    squares exact): which statistics of a forward may be compared."""
    pl, pt, oh, ow = geom(cs)
    assert survives_storage(r.e) and survives_storage(r.dy)
    assert torch.equal(r.wk, r.wk.float().double()) and float(r.wk.abs().max()) <= 3
    if cs.sat:
        assert survives_storage(r.e + SHIFT)
    stats = (False, False)
    if cs.kind == "fwd":
        assert survives_storage(r.y), "an output does not survive the storage type"
        assert float(r.y.abs().max()) <= (75 if not cs.sat else 500 if cs.k == 5 else 360)
        stats = (float(r.y.abs().sum((0, 1, 2)).max()) < TWO24, float((r.y * r.y).sum((0, 1, 2)).max()) < TWO24)
        if not cs.sat and cs.seam != "ring":
            assert all(stats), "a plain forward compares both statistics"
    if cs.kind in ("gather", "dgrad2", "dgrad1", "fused"):
        assert survives_storage(r.dx) and float(r.dx.abs().max()) <= 75
        assert float(r.dx.abs().sum((0, 1, 2)).max()) < TWO24          # sum dZ0 and sum dZ0 * e: |terms| = |dZ0|
    if cs.kind in ("wgrad", "fused"):
        assert (20 if cs.sat else 1) * cs.n * oh * ow < TWO24            # |dW| <= sum |dy * a0|: every partial sum is exact
        assert float(r.dw.abs().max()) + 64 < TWO24                      # (+ the integer prefill the launch accumulates into)
    return stats


# ------------------------------------------------------------------------------------------------------------ routes
def dw_args(cs, launch):
    """the argument block (geometry fields only) of the launch a case makes; launch in conv (the conv's own geometry: forward,
    weight gradient, mc_dwconv_bwd_data) or flipped (the stride-1 data gradient / fused backward: a forward on the conv's output
    geometry with pads k - 1 - pad)"""
    pl, pt, oh, ow = geom(cs)
    a = L.DwconvArgs()
    if launch == "conv":
        a.n, a.h, a.w, a.c, a.k, a.stride, a.pad_l, a.pad_t, a.oh, a.ow = cs.n, cs.h, cs.w, cs.c, cs.k, cs.s, pl, pt, oh, ow
    else:
        assert cs.s == 1
        a.n, a.h, a.w, a.c, a.k, a.stride, a.pad_l, a.pad_t, a.oh, a.ow = cs.n, oh, ow, cs.c, cs.k, 1, cs.k - 1 - pl, cs.k - 1 - pt, cs.h, cs.w
    return a


LANE_MODE = {"fwd": 0, "dgrad1": 1, "wgrad": 2, "fused": 3}


def lane_blocks(cs, p):
    """the largest number of 4-input-row blocks a workgroup of the lane = column launch walks: the kernel's range arithmetic
    (conv_lane.hip: virtual rows [vt * y / ycp, vt * (y + 1) / ycp) of (image group, strip, output row))"""
    oh = geom(cs)[2]                                       # (the stride-1 launches on flipped taps: the same number)
    nblk = lambda rows: ((rows - 1) * cs.s + cs.k + 3) // 4
    vt = -(-cs.n // p["G"]) * p["strips"] * oh
    most = 0
    for cpair in range(p["cpairs"]):
        ycp = (p["nunits"] - cpair + p["cpairs"] - 1) // p["cpairs"]
        for y in range(ycp):
            v0, v1 = vt * y // ycp, vt * (y + 1) // ycp
            u0, u1 = v0 // oh, v1 // oh
            o0, o1 = v0 - u0 * oh, v1 - u1 * oh
            nr0 = o1 - o0 if u0 == u1 else oh - o0
            tot = (nblk(nr0) if nr0 > 0 else 0) + max(u1 - u0 - 1, 0) * nblk(oh) + (nblk(o1) if u1 > u0 and o1 > 0 else 0)
            most = max(most, tot)
    return most


def route(cs):
    """what the library's host queries say about the launch of a case: a dict of plan values (+ "rows": the query's return)"""
    lib = L.load()
    pl, pt, oh, ow = geom(cs)
    if cs.kind == "gather":
        total = cs.n * cs.h * cs.w * (cs.c // 8)
        return dict(blocks=-(-total // 256), ragged=int(total % 256 != 0), rows=0)
    if cs.kind == "dgrad2":
        a = dw_args(cs, "conv")
        a.epi_x = 16
        plan = (C.c_int * 4)()
        rows = lib.mc_dwconv_bwd_data_plan(C.byref(a), plan)
        p = dict(zip(("strips", "segs", "seg_rows", "ctiles"), plan), rows=rows)
        if not cs.sat:
            # the launch without the epilogue stages longer blocks (at most 8 super-rows) and cuts its segments in whole blocks:
            # the query answers for the epilogue form, so hold the plain form to the longest segments it can have (march_segments
            # in conv.hip: enough segments for 2048 items, none shorter than 16 super-rows, rounded up to whole blocks)
            ohv = (cs.h + pt + 1) >> 1
            asked = min(max(ohv // 16, 1), -(-2048 // (cs.n * p["strips"] * p["ctiles"])))
            p["segs"] = min(p["segs"], -(-ohv // (-(-ohv // asked) + 7)))
        return p
    if cs.lane:
        a = dw_args(cs, "conv" if cs.kind in ("fwd", "wgrad") else "flipped")
        plan = (C.c_int * 8)()
        rows = lib.mc_dwconv_lane_plan(C.byref(a), LANE_MODE[cs.kind], plan)
        p = dict(zip(("G", "ncol", "tow", "strips", "ctiles", "cpairs", "nunits", "ymax"), plan), rows=rows)
        p["blocks"] = lane_blocks(cs, p)
        p["xmap"] = int(p["nunits"] % 8 == 0)
        p["slot_fewer"] = int(p["nunits"] % p["cpairs"] != 0)
        return p
    a = dw_args(cs, "conv" if cs.kind in ("fwd", "wgrad") else "flipped")
    if cs.kind == "dgrad1":
        a.epi_x = 16
    plan = (C.c_int * 6)()
    rows = lib.mc_dwconv_march_plan(C.byref(a), int(cs.kind == "wgrad"), plan)
    return dict(zip(("tow", "tch", "strips", "segs", "seg_rows", "gy"), plan), rows=rows)


def check_route(cs, p):
    assert cs.want, "every row names what it must reach"
    for name, v in cs.want.items():
        if isinstance(v, tuple):
            assert v[0] == ">=" and p[name] >= v[1], (case_id(cs), name, p[name], v)
        else:
            assert p[name] == v, (case_id(cs), name, p[name], v)


# ------------------------------------------------------------------------------------------------------------ tables
CASES = []


def add(kinds, lane, k, s, n, h, w, c, seam, **want):
    """kinds: names with an optional "+sat" -- one row per name"""
    for kd in kinds.split():
        kind, _, sat = kd.partition("+")
        CASES.append(Case(kind, lane, k, s, n, h, w, c, sat == "sat", seam, want))


def in_size(out, s, odd):
    """an input size whose "same" conv of stride s has `out` outputs; odd: the other pad form of stride 2"""
    return out if s == 1 else 2 * out - (1 if odd else 0)


# ---- marching kernels (lane mode 0).  (k, s, c) -> (strip width, channels per tile): MarchCfg / march_dispatch in conv.hip
MARCH_TILES = [(3, 1, 24, 80, 24), (3, 2, 24, 80, 24), (3, 1, 48, 40, 48), (3, 2, 144, 40, 48), (3, 1, 64, 32, 64), (3, 2, 72, 32, 64),
               (3, 1, 240, 8, 240), (5, 1, 64, 32, 64), (5, 1, 40, 32, 64), (5, 2, 40, 16, 64)]
FW = "fwd fwd+sat wgrad wgrad+sat"
for k, s, c, tow, tch in MARCH_TILES:
    # a second strip of one column; a middle strip with halo columns on both sides
    add(FW, 0, k, s, 2, in_size(5, s, False), in_size(tow + 1, s, False), c, "strip+1", tow=tow, tch=tch, strips=2, segs=1)
    add(FW, 0, k, s, 2, in_size(5, s, True), in_size(2 * tow + 1, s, True), c, "strip-mid", tow=tow, tch=tch, strips=3, segs=1)
# row segments (n = 1: from 48 output rows up, 24 rows at least): two and three, the last one ragged; one strip
for k in (3, 5):
    for s in (1, 2):
        add(FW, 0, k, s, 1, in_size(49, s, k == 5), in_size(9, s, k == 3), 16, "segs2", strips=1, segs=2)
        add(FW, 0, k, s, 1, in_size(75, s, k == 3), in_size(9, s, k == 5), 16, "segs3", strips=1, segs=3)
add(FW, 0, 3, 1, 1, 49, 33, 64, "strips2xsegs2", strips=2, segs=2)
add(FW, 0, 5, 2, 1, 98, 34, 40, "strips2xsegs2", strips=2, segs=2)
# the stride-1 gather data gradient: a ragged last workgroup
add("gather", 0, 3, 1, 1, 7, 9, 40, "ragged-wg", blocks=2, ragged=1)
add("gather", 0, 5, 1, 2, 5, 11, 24, "ragged-wg", blocks=2, ragged=1)
# the stride-2 data gradient, plain and with the saturated epilogue, both pad forms: >= 2 strips and >= 2 segments at the three
# tile shapes (48- and 64-channel tiles of 3x3: 20 / 16 super-columns per strip; 5x5: 16)
for k, c, w in ((3, 48, 82), (3, 72, 66), (5, 40, 66)):
    for odd in (0, 1):
        add("dgrad2 dgrad2+sat", 0, k, 2, 1, 66 + odd, w + odd, c, "s2-strips-segs", strips=(">=", 2), segs=(">=", 2), ctiles=-(-c // (48 if c == 48 else 64)))
# the stride-1 data gradient on flipped taps with the saturated epilogue: a strip seam, a segment seam
add("dgrad1+sat", 0, 3, 1, 2, 5, 33, 64, "strip+1", tow=32, strips=2, segs=1)
add("dgrad1+sat", 0, 5, 1, 2, 5, 65, 40, "strip-mid", tow=32, strips=3, segs=1)
add("dgrad1+sat", 0, 3, 1, 1, 49, 9, 48, "segs2", strips=1, segs=2)
add("dgrad1+sat", 0, 5, 1, 1, 75, 9, 16, "segs3", strips=1, segs=3)

# ---- lane = column kernels (lane mode 1).  Strip widths / image-group thresholds: Cfg<K, S, NCOL, G>::TOW in conv_lane.hip
TWO_COL = {3: (126, 62, 30), 5: (124, 60, 29)}                         # k -> TOW of G = 1, 2, 4 (two output columns per lane, stride 1)
ONE_COL = {(3, 1): (62, 30), (5, 1): (60, 29), (3, 2): (63, 31), (5, 2): (62, 30)}     # (k, s) -> TOW of G = 1, 2 (one column per lane)
S1 = "fwd fwd+sat dgrad1+sat wgrad wgrad+sat fused+sat"
S2 = "fwd fwd+sat wgrad wgrad+sat"


def one_col(kind, k, s):
    return s == 2 or kind == "fused" or (kind == "wgrad" and k == 5)


def lane_config(kind, k, s, n, ow):
    """(G, columns per lane, strip width, strips) from the tables above, as lane::pick / lane::plan choose them"""
    if one_col(kind, k, s):
        t1, t2 = ONE_COL[(k, s)]
        return (2, 1, t2, 1) if n >= 2 and ow <= t2 else (1, 1, t1, -(-ow // t1))
    t1, t2, t4 = TWO_COL[k]
    if n >= 4 and ow <= t4:
        return 4, 2, t4, 1
    if n >= 2 and ow <= t2:
        return 2, 2, t2, 1
    if ow <= ONE_COL[(k, s)][0]:
        return 1, 1, ONE_COL[(k, s)][0], 1
    return 1, 2, t1, -(-ow // t1)


def add_lane(kinds, k, s, n, h, w, c, seam, need=None, **want):
    """one row per kind; G, columns per lane, strip width and strip count always asserted; need(G, ncol, tow, strips) says
    whether the configuration a kind gets reaches the seam the row is there for (else the kind is left out)"""
    ow = same_pad(w, k, s)[1]
    for kd in kinds.split():
        kind = kd.partition("+")[0]
        G, ncol, tow, strips = lane_config(kind, k, s, n, ow)
        if need is None or need(G, ncol, tow, strips):
            add(kd, 1, k, s, n, h, w, c, seam, **dict(dict(G=G, ncol=ncol, tow=tow, strips=strips), **want))


for k in (3, 5):
    t1, t2, t4 = TWO_COL[k]
    o1, o2 = ONE_COL[(k, 1)]
    # one-image strips: a second strip of one column, two-column and one-column configurations
    add_lane(S1, k, 1, 1, 6, t1 + 1, 40, "strip+1", lambda G, ncol, tow, strips: ncol == 2 and strips == 2 and G == 1)
    add_lane(S1, k, 1, 1, 6, o1 + 1, 40, "strip+1", lambda G, ncol, tow, strips: ncol == 1 and strips == 2 and G == 1)
    # image groups: at each width threshold and one column narrower; 29 columns of 5x5: the 33-column segment
    for wd in (t4, t4 - 1):
        add_lane(S1, k, 1, 4, 7, wd, 40, "group", lambda G, ncol, tow, strips: G == (4 if ncol == 2 else 2))
        add_lane(S1, k, 1, 5, 5, wd, 8, "group-ragged", lambda G, ncol, tow, strips: G == (4 if ncol == 2 else 2))
    for wd in (t2, t2 - 1):
        add_lane(S1, k, 1, 2, 7, wd, 40, "group", lambda G, ncol, tow, strips: G == 2)
        add_lane(S1, k, 1, 3, 5, wd, 8, "group-ragged", lambda G, ncol, tow, strips: G == 2)
    for wd in (o2, o2 - 1):
        add_lane(S1, k, 1, 3, 5, wd, 8, "group-ragged", lambda G, ncol, tow, strips: G == 2 and ncol == 1)
    # just past a threshold: fewer images per wave
    add_lane(S1, k, 1, 4, 5, t4 + 1, 8, "past-G4", lambda G, ncol, tow, strips: ncol == 2 and G == 2)
    add_lane(S1, k, 1, 2, 5, t2 + 1, 8, "past-G2", lambda G, ncol, tow, strips: ncol == 2 and G == 1)
    add_lane(S1, k, 1, 2, 5, o2 + 1, 8, "past-G2", lambda G, ncol, tow, strips: ncol == 1 and G == 1)
    # unit ranges (a workgroup gets at least 8 virtual rows): three units that begin in the middle of an image; units that
    # straddle image boundaries; 8 units = the contiguous XCD mapping (the others: the modulo mapping)
    add_lane(S1, k, 1, 1, 24, 20, 8, "units-mid-image", nunits=3, xmap=0)
    add_lane(S1, k, 1, 3, 11, 64, 8, "units-straddle", lambda G, ncol, tow, strips: strips == 1, nunits=4, xmap=0)
    add_lane(S1, k, 1, 3, 11, 64, 8, "units-straddle", lambda G, ncol, tow, strips: strips == 2, nunits=8, xmap=1)
    add_lane(S1, k, 1, 1, 64, 20, 8, "xcd-contiguous", nunits=8, xmap=1)
    # more than 128 blocks of 4 input rows in one workgroup: the descriptor ring is refilled
    add_lane("fwd dgrad1+sat wgrad fused+sat", k, 1, 1, 66000, 5, 8, "ring", nunits=128, blocks=(">=", 129))
for k in (3, 5):
    for s in (2,):
        o1, o2 = ONE_COL[(k, s)]
        add_lane(S2, k, s, 1, 12, in_size(o1 + 1, s, k == 5), 40, "strip+1", lambda G, ncol, tow, strips: strips == 2)
        for i, wd in enumerate((o2, o2 - 1)):
            add_lane(S2, k, s, 2, in_size(7, s, i == 0), in_size(wd, s, i == 1), 40, "group", lambda G, ncol, tow, strips: G == 2)
            add_lane(S2, k, s, 3, in_size(5, s, i == 1), in_size(wd, s, i == 0), 8, "group-ragged", lambda G, ncol, tow, strips: G == 2)
        add_lane(S2, k, s, 2, 10, in_size(o2 + 1, s, False), 8, "past-G2", lambda G, ncol, tow, strips: G == 1)
        add_lane(S2, k, s, 1, 48, 40, 8, "units-mid-image", nunits=3, xmap=0)
        add_lane(S2, k, s, 1, 127, 39, 8, "xcd-contiguous", nunits=8, xmap=1)
# channel tiles.  16 waves (32-channel tiles): one ragged tile (c = 8, above); a pair with a ragged second tile (c = 40, above);
# three tiles: the second pair's second tile is absent.  12 waves (the fused 5x5, 24-channel tiles): 24, 32, 56
for k in (3, 5):
    add_lane("fwd fwd+sat dgrad1+sat wgrad wgrad+sat" + (" fused+sat" if k == 3 else ""), k, 1, 2, 16, 20, 72, "tiles3", ctiles=3, cpairs=2, nunits=4)
    add_lane(S2, k, 2, 2, 32, 40, 72, "tiles3", ctiles=3, cpairs=2, nunits=4)
for c, ct in ((24, 1), (32, 2), (56, 3)):
    add_lane("fused+sat", 5, 1, 2, 16, 20, c, "tiles12w", ctiles=ct, cpairs=(ct + 1) // 2)
# a tile pair with one y slot fewer than the others (the 128-unit cap on three tile pairs): its extra partial rows are zeros
for k in (3, 5):
    add_lane("fwd fwd+sat dgrad1+sat wgrad wgrad+sat" + (" fused+sat" if k == 3 else ""), k, 1, 1, 344, 4, 160, "slot-fewer", ctiles=5, cpairs=3, nunits=128, slot_fewer=1)
add_lane("fused+sat", 5, 1, 1, 344, 4, 120, "slot-fewer", ctiles=5, cpairs=3, nunits=128, slot_fewer=1)

# the same geometry in consecutive rows: one reference serves them
CASES.sort(key=lambda cs: (cs.k, cs.s, cs.n, cs.h, cs.w, cs.c, cs.sat))
assert len({case_id(cs) for cs in CASES}) == len(CASES)
