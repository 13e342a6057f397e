"""Training augmentation without a GPU: the host path of mammo_clip_amd/augment.py (the integer specification, executable)
against exact expectations and against scipy's fp64 filters, the sampler, and the argument checks of mc_augment_u8."""
import ctypes
import math

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from mammo_clip_amd import augment as A
from mammo_clip_amd import lib as L


def _img(h, w, seed=0, n=1):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)


def _one(src, row, sigma=1.0):
    out = A.augment(src, np.asarray([row], dtype=np.int32), sigma)
    assert out.shape == (1, 3) + src.shape[1:] and out.dtype == np.uint8
    assert np.array_equal(out[0, 0], out[0, 1]) and np.array_equal(out[0, 0], out[0, 2])
    return out[0, 0]


def _row(idx=0, flags=0, m=(65536, 0, 0, 65536), b=(0, 0), alpha_q8=0, seed=(0, 0)):
    return [idx, flags, *m, *b, alpha_q8, *seed, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ Philox
def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32-10"""
    assert [int(w) for w in A.philox4x32(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert [int(w) for w in A.philox4x32(f, f, f, f, f, f)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_noise_layout_eight_values_per_counter():
    n = A.noise(5, 7, 11, 22, 1)                                 # 35 values: counters 0..4
    w = A.philox4x32(np.arange(5), 0, 1, 0x5bd1e995, 11, 22)
    flat = n.reshape(-1)
    for i in (0, 1, 6, 7, 8, 21, 34):
        word = int(w[(i & 7) >> 1][i >> 3])
        half = (word >> 16) if i & 1 else (word & 0xffff)
        assert flat[i] == half - 32768


# ------------------------------------------------------------------------------------------------ exact cases
def test_identity_row_returns_the_source_in_all_planes():
    src = _img(67, 45, n=3)
    out = A.augment(src, A.identity_rows(3), 2.0)
    for c in range(3):
        assert np.array_equal(out[:, c], src)


@pytest.mark.parametrize("flags,axes", [(1, (1,)), (2, (0,)), (3, (0, 1))])
def test_flips_alone_are_np_flip(flags, axes):
    src = _img(12, 9)
    assert np.array_equal(_one(src, _row(flags=flags)), np.flip(src[0], axes))


def test_integer_translation_exposes_zeros():
    src = _img(14, 11)
    tx, ty = 3, -2                                               # output(x, y) = source(x - tx, y - ty)
    got = _one(src, _row(b=(-tx << 16, -ty << 16)))
    want = np.zeros_like(src[0])
    want[:14 + ty, tx:] = src[0][-ty:, :11 - tx]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", [1, -1])
def test_quarter_turn_about_the_centre_of_an_odd_square(k):
    n = 13
    src = _img(n, n)
    c = (n - 1) // 2
    # np.rot90 (counter-clockwise, k = 1): out[y, x] = src[x, n-1-y], i.e. sx = n-1-y, sy = x; about the centre that is the
    # inverse matrix [[0, -1], [1, 0]] with b = c - M c; k = -1 is its transpose
    m = (0, -65536, 65536, 0) if k == 1 else (0, 65536, -65536, 0)
    b = ((c - (m[0] * c + m[1] * c) // 65536) << 16, (c - (m[2] * c + m[3] * c) // 65536) << 16)
    assert np.array_equal(_one(src, _row(m=m, b=b)), np.rot90(src[0], k))


# ------------------------------------------------------------------------------------------------ general affine
def _smooth(h, w):
    """uint8 image in [0, 127] whose horizontally / vertically neighbouring pixels differ by at most 7 levels"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = 63.5 + 28.0 * np.sin(x / 9.0) * np.cos(y / 11.0) + 28.0 * np.sin((x + 2.0 * y) / 17.0)
    img = np.rint(f).astype(np.uint8)
    d0, d1 = np.abs(np.diff(img.astype(int), axis=0)).max(), np.abs(np.diff(img.astype(int), axis=1)).max()
    assert 4 <= max(d0, d1) <= 7 and img.max() <= 127
    return img


def test_general_affine_against_fp64_bilinear():
    """20 seeded draws from the reference's ranges against scipy.ndimage.map_coordinates(order=1) in fp64 with the
    unquantised inverse matrix.  Where all four taps lie inside the source the reference is mode="constant"; elsewhere it is
    mode="grid-constant": "constant" returns 0 for every coordinate outside [0, n-1] and never blends with the border, while
    the specification reads a tap outside as 0 -- "grid-constant" is that rule in scipy (the two modes agree inside).
    Bound.  Source coordinate error per axis: Q8 rounding 2^-9, the rs(., 16) rounding 2^-17, the Q16 matrix and translation
    (|x| + |y| + 1) 2^-17 <= 228 x 2^-17: e <= 0.0037 px.  Times the bilinear surface's slope -- 7 levels / px per axis
    inside, up to 127 levels / px per axis where a tap is the zero border -- plus 0.5 for the final rounding:
    0.0037 x 14 + 0.5 < 1 inside, 0.0037 x 254 + 0.5 < 2 elsewhere."""
    H, W = 130, 97
    img = _smooth(H, W)
    rng = np.random.default_rng(7)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    worst_in, worst_rim = 0.0, 0.0
    for _ in range(20):
        fwd = A.affine_matrix(rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2),
                              rng.uniform(-0.1, 0.1) * W, rng.uniform(-0.1, 0.1) * H, H, W)
        inv = np.linalg.inv(fwd)
        m = [int(v) for v in np.rint(inv[:2, :2] * 65536).reshape(-1)]
        b = [int(v) for v in np.rint(inv[:2, 2] * 65536)]
        got = _one(img[None], _row(m=m, b=b)).astype(np.float64)
        sx = inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2]
        sy = inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2]
        ref = ndi.map_coordinates(img.astype(np.float64), [sy, sx], order=1, mode="constant", cval=0.0)
        ref_rim = ndi.map_coordinates(img.astype(np.float64), [sy, sx], order=1, mode="grid-constant", cval=0.0)
        fx, fy = np.floor(sx), np.floor(sy)
        inside = (fx >= 0) & (fx + 1 <= W - 1) & (fy >= 0) & (fy + 1 <= H - 1)
        assert inside.sum() > 0.5 * H * W and (~inside).sum() > 100
        e_in, e_rim = np.abs(got - ref)[inside].max(), np.abs(got - ref_rim)[~inside].max()
        worst_in, worst_rim = max(worst_in, e_in), max(worst_rim, e_rim)
        assert e_in <= 1.0 and e_rim <= 2.0, (e_in, e_rim)
    print(f"affine vs fp64: max inside {worst_in:.3f}, elsewhere {worst_rim:.3f}")


# ------------------------------------------------------------------------------------------------ field
@pytest.mark.parametrize("H,W,sigma", [(61, 61, 15.0), (130, 97, 3.0), (200, 333, 6.5)])
def test_field_against_scipy_gaussian_filter(H, W, sigma):
    """v / 2^30 vs gaussian_filter(n / 32768) in fp64.  Bound: each of the 2R + 1 taps is rounded to 2^-15 of its sum (error
    <= 2^-16 each per pass, two passes, |n| <= 1: (2R + 1) 2^-15), plus the int16 rounding of h (2^-16 of full scale, through
    taps that sum to one) -- (2R + 1) 2^-15 + 2^-15."""
    taps = A.gaussian_taps(sigma, H, W)
    R = (taps.size - 1) // 2
    assert R == int(4 * sigma + 0.5) and int(taps.sum()) == 32768 and (taps[:R] == taps[:R:-1]).all()
    for comp in (0, 1):
        n = A.noise(H, W, 0x1234, 0xabcd, comp)
        h, v = A.field(H, W, taps, 0x1234, 0xabcd, comp)
        assert np.abs(h).max() < 2 ** 15 and np.abs(v).max() < 2 ** 31
        ref = ndi.gaussian_filter(n / 32768.0, sigma, mode="mirror", truncate=4.0)
        err = np.abs(v / 2.0 ** 30 - ref).max()
        print(f"field {H}x{W} sigma {sigma} comp {comp}: max error {err:.3e}")
        assert err <= (2 * R + 1) * 2.0 ** -15 + 2.0 ** -15


def test_elastic_displacement_is_alpha_times_the_blurred_noise():
    """elastic alone on a horizontal ramp: out(x, y) ~ ramp(x + dx), dx = alpha blur(noise / 32768)"""
    H, W, sigma, alpha = 40, 50, 2.0, 64.0
    src = np.broadcast_to((np.arange(W) * 5).astype(np.uint8), (1, H, W)).copy()
    got = _one(src, _row(flags=4, alpha_q8=int(alpha * 256), seed=(5, 6)), sigma).astype(np.float64)
    dx = alpha * ndi.gaussian_filter(A.noise(H, W, 5, 6, 0) / 32768.0, sigma, mode="mirror", truncate=4.0)
    x = np.arange(W)[None, :] + dx
    x = np.abs(x)
    x = np.where(x > W - 1, 2 * (W - 1) - x, x)
    # ramp slope 5 levels / px; displacement error alpha (2R + 2) 2^-15 px + 2^-9 px of Q8 rounding, + 0.5 final rounding
    tol = 5 * (alpha * (2 * 8 + 2) * 2.0 ** -15 + 2.0 ** -9) + 0.5
    assert np.abs(got - 5 * x).max() <= tol and np.abs(dx).max() > 1.0


# ------------------------------------------------------------------------------------------------ ranges and errors
def test_ranges_and_errors():
    src = _img(20, 30)
    with pytest.raises(ValueError):
        A.augment(src, A.identity_rows(1), 0.49)                # sigma < 0.5
    with pytest.raises(ValueError):
        A.augment(src, A.identity_rows(1), 5.0)                 # R = 20 > min(H, W) - 1 = 19
    A.augment(src, A.identity_rows(1), 4.75)                    # R = 19: the largest allowed
    with pytest.raises(ValueError):
        A.augment(_img(300, 300), A.identity_rows(1), 32.2)     # R = 129 > 128
    with pytest.raises(ValueError):
        A.augment(src, np.asarray([_row(flags=4, alpha_q8=256 * 256 + 1)], dtype=np.int32), 1.0)
    A.augment(src, np.asarray([_row(flags=4, alpha_q8=256 * 256)], dtype=np.int32), 1.0)
    for idx in (-1, 1):
        with pytest.raises(ValueError):
            A.augment(src, np.asarray([_row(idx=idx)], dtype=np.int32), 1.0)
    with pytest.raises(ValueError):
        A.AugmentPolicy(alpha=257.0)


def test_strided_source_and_tensor_input():
    hwc = np.random.default_rng(3).integers(0, 256, (2, 9, 7, 3), dtype=np.uint8)
    rows = np.asarray([_row(idx=1, flags=1), _row(idx=1)], dtype=np.int32)
    a = A.augment(hwc[..., 1], rows, 1.0)
    b = A.augment(np.ascontiguousarray(hwc[..., 1]), rows, 1.0)
    t = A.augment(torch.from_numpy(hwc)[..., 1], torch.from_numpy(rows), 1.0)
    assert np.array_equal(a, b) and torch.is_tensor(t) and np.array_equal(t.numpy(), a)
    assert np.array_equal(a[1, 0], hwc[1, :, :, 1])


# ------------------------------------------------------------------------------------------------ sampler
REF_CFG = {"affine_transform_degree": 20, "affine_translate_percent": 0.1, "affine_scale": [0.8, 1.2], "affine_shear": 20,
           "elastic_transform_alpha": 10, "elastic_transform_sigma": 15, "p": 1.0}


def test_sampler_rows_lie_inside_the_ranges():
    pol = A.AugmentPolicy.from_transform_config({"train": {"transform": REF_CFG}})
    assert (pol.alpha, pol.sigma, pol.size) == (10.0, 15.0, (1520, 912))
    g = torch.Generator().manual_seed(0)
    n, (H, W) = 400, pol.size
    state = g.get_state()
    d = pol.draw(n, g)
    assert np.abs(d["rotate"]).max() <= 20 and np.abs(d["shear"]).max() <= 20
    assert np.abs(d["translate_x"]).max() <= 0.1 and np.abs(d["translate_y"]).max() <= 0.1
    for k in ("scale_x", "scale_y"):
        assert 0.8 <= d[k].min() and d[k].max() <= 1.2
    for k in ("hflip", "vflip", "affine", "elastic"):           # p = 0.5 each: 400 draws stay within 6 sigma of 200
        assert 140 < int(d[k].sum()) < 260
    g.set_state(state)
    rows = pol.sample(n, g)
    assert rows.dtype == np.int32 and rows.shape == (n, 16) and not rows[:, 11:].any() and not (rows[:, 1] & ~7).any()
    assert np.array_equal(rows[:, 1] & 4 != 0, d["elastic"]) and np.array_equal(rows[:, 0], np.arange(n))
    assert set(np.unique(rows[:, 8])) == {0, 2560} and np.array_equal(rows[:, 8] != 0, d["elastic"])
    assert len({(int(a), int(b)) for a, b in rows[:, 9:11]}) == n  # a fresh seed per row
    ident = A.identity_rows(1)[0, 2:8]
    for i in range(n):
        if not d["affine"][i]:
            assert np.array_equal(rows[i, 2:8], ident)
            continue
        # the quantised inverse undoes the forward matrix of the drawn parameters: |M_q16 F - I| within the Q16 rounding
        fwd = A.affine_matrix(d["rotate"][i], d["shear"][i], d["scale_x"][i], d["scale_y"][i], d["translate_x"][i] * W,
                              d["translate_y"][i] * H, H, W)
        inv = np.eye(3)
        inv[:2, :2] = rows[i, 2:6].reshape(2, 2) / 65536.0
        inv[:2, 2] = rows[i, 6:8] / 65536.0
        prod = inv @ fwd
        assert np.abs(prod[:2, :2] - np.eye(2)).max() <= 4 * 2.0 ** -17 * 1.5
        assert np.abs(prod[:2, 2]).max() <= 2.0 ** -17 * (2 * 1.5 * max(H, W) + 1)
        # singular values of the inverse's linear part: 1 / scale, stretched by the shear (tan 20 deg) at most
        sv = np.linalg.svd(inv[:2, :2], compute_uv=False)
        k = math.tan(math.radians(20))
        stretch = (k + math.sqrt(k * k + 4)) / 2
        assert 1 / (1.2 * stretch) - 1e-4 <= sv.min() and sv.max() <= stretch / 0.8 + 1e-4


def test_sampler_p_zero_gives_identity_rows_only():
    pol = A.AugmentPolicy.from_transform_config(dict(REF_CFG, p=0.0), size=(64, 48))
    rows = pol.sample(50, torch.Generator().manual_seed(1))
    assert np.array_equal(rows[:, :9], A.identity_rows(50)[:, :9])


def test_sampler_is_a_function_of_the_generator_state():
    pol = A.AugmentPolicy.from_transform_config(REF_CFG, size=(64, 48))
    a = pol.sample(16, torch.Generator().manual_seed(5))
    b = pol.sample(16, torch.Generator().manual_seed(5))
    c = pol.sample(16, torch.Generator().manual_seed(6))
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_the_two_views_of_a_pair_differ():
    pol = A.AugmentPolicy.from_transform_config(REF_CFG, size=(64, 48))
    g = torch.Generator().manual_seed(2)
    first, second = pol.sample(8, g), pol.sample(8, g)
    assert np.array_equal(first[:, 0], second[:, 0])
    assert all(not np.array_equal(first[i, 1:], second[i, 1:]) for i in range(8))


# ------------------------------------------------------------------------------------------------ ABI
def test_augment_entry_points_validate_arguments_without_gpu():
    lib = L.load()
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)                                    # non-null, never dereferenced: the checks come first
    one = lib.mc_augment_ws_bytes(1, 61, 45)
    assert one >= 2 * 2 * 61 * 45 and lib.mc_augment_ws_bytes(7, 61, 45) == 7 * one
    assert lib.mc_augment_ws_bytes(0, 61, 45) == 0 and lib.mc_augment_ws_bytes(1, 0, 45) == 0
    assert lib.mc_augment_ws_bytes(1, 16385, 45) == 0

    def call(src=p, params=p, taps=p, dst=p, ws=p, n_src=1, n_out=1, radius=2, h=61, w=45, ws_bytes=one):
        return lib.mc_augment_u8(src, 61 * 45, 45, 1, n_src, params, n_out, taps, radius, h, w, dst, ws, ws_bytes, None)

    for kw in ({"src": None}, {"params": None}, {"taps": None}, {"dst": None}, {"ws": None}):
        assert call(**kw) != 0 and b"augment_u8: null" in lib.mc_last_error(), kw
    for kw in ({"radius": 0}, {"radius": 129, "h": 300, "w": 300, "ws_bytes": 1 << 30}, {"radius": 45}):
        assert call(**kw) != 0 and b"radius" in lib.mc_last_error(), kw
    for kw in ({"h": 0}, {"w": 0}, {"h": 16385}):
        assert call(**kw) != 0 and b"extents" in lib.mc_last_error(), kw
    assert call(ws_bytes=one - 1) != 0 and b"ws_bytes" in lib.mc_last_error()
    assert call(n_out=0) != 0 and call(n_src=0) != 0
