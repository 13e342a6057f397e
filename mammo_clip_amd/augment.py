"""Training augmentation on the device: both image views of a pair from ONE uint8 grayscale upload.

The reference's training transform [ref: data/data_utils.py:25-62] is albumentations'
``Compose([HorizontalFlip, VerticalFlip, Affine, ElasticTransform], p)``, applied twice per sample (``image`` and
``image_view``) [ref: data/datasets/imagetext.py:126-160].  Here the composition elastic o affine o flips is ONE gather with
the library's documented borders (constant 0 for Affine, reflect-101 for ElasticTransform), written as an integer
specification that the host path of this module (plain numpy, int64) and the HIP kernels (csrc/augment.hip) both implement
exactly: the device is tested against the host byte for byte.  It is deliberately NOT bit-compatible with albumentations /
OpenCV (three resamplings there, one here; another RNG) and cannot be checked to be: neither library is a dependency.

Specification.  ``rs(a, s) = (a + (1 << (s-1))) >> s`` with an arithmetic shift; W, H are the image extents, (x, y) an output
pixel.

Per output image, one row of 16 int32:
    0      source image index
    1      flags: bit 0 horizontal flip, bit 1 vertical flip, bit 2 elastic on
    2-5    m00 m01 m10 m11: inverse affine matrix (output -> source), Q16
    6-7    b0 b1: inverse translation, Q16 pixels
    8      alpha_q8 = round(alpha * 256), 0 <= alpha <= 256
    9-10   low and high word of a 64-bit seed
    11-15  zero

Per call: sigma >= 0.5 becomes a tap table built on the host in fp64: R = int(4 sigma + 0.5),
g[t] = rint(32768 exp(-t^2 / 2 sigma^2) / sum) for t = -R..R, the centre tap corrected so that sum g = 32768 exactly;
R <= min(H, W) - 1 and R <= 128, anything else raises.

Noise: for component c (0 = dx, 1 = dy) and i = y W + x the word is
``philox4x32(lo32(i >> 3), hi32(i >> 3), c, 0x5bd1e995, seed_lo, seed_hi)[(i & 7) >> 1]``; the half is the low 16 bits when
i is even, else the high 16 bits; n = half - 32768.

Field: h = rs(sum_t g[t] n(y, refl(x + t, W)), 15) (fits int16); v = sum_t g[t] h(refl(y + t, H), x) (fits int32);
refl(i, n) is reflect-101 with a single fold: i <- |i|, then 2(n-1) - i if i > n-1.  d = rs(alpha_q8 v, 22) with a 64-bit
product: the displacement in Q16 pixels, alpha * blur(noise / 32768).

Map: qx = (x << 16) + dx, qy = (y << 16) + dy (dx = dy = 0 when flags bit 2 is clear).  With the elastic on each of qx, qy is
folded once by reflect-101 at L = (extent - 1) << 16, then clamped to [0, L].  rx = rs(m00 qx + m01 qy, 16) + b0 and
ry = rs(m10 qx + m11 qy, 16) + b1 with 64-bit products; sx = rs(rx, 8), sy = rs(ry, 8) in Q8.  Flips apply to the source:
sx <- ((W-1) << 8) - sx for a horizontal flip, sy <- ((H-1) << 8) - sy for a vertical one.  ix = sx >> 8, fx = sx & 255,
likewise for y.

Sample: the four taps are a = (iy, ix), b = (iy, ix+1), c = (iy+1, ix), d = (iy+1, ix+1); a tap outside the source reads 0.
out = rs((256-fx)(256-fy) a + fx (256-fy) b + (256-fx) fy c + fx fy d, 16), written to all three channel planes.
"""
import math

import numpy as np

ROW = 16                      # int32 values per output image
FLAG_HFLIP, FLAG_VFLIP, FLAG_ELASTIC = 1, 2, 4
MAX_RADIUS = 128
MAX_EXTENT = 16384            # (extent - 1) << 16 plus a displacement stays inside int32

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123).  Counter words are arrays or ints, the key two ints; returns four uint64 arrays holding
    32-bit words.  The same function as ``philox4x32`` of csrc/common_hip.h."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def rs(a, s):
    """rounding arithmetic shift of the specification"""
    return (a + (1 << (s - 1))) >> s


def gaussian_taps(sigma, height, width):
    """int32 [2R+1] taps of the call (sum = 32768) for ``sigma``; raises where the specification does"""
    sigma = float(sigma)
    if not sigma >= 0.5:
        raise ValueError(f"augment: sigma must be >= 0.5, got {sigma}")
    radius = int(4.0 * sigma + 0.5)
    if radius > MAX_RADIUS or radius > min(height, width) - 1:
        raise ValueError(f"augment: radius {radius} of sigma {sigma} exceeds min({MAX_RADIUS}, min(H, W) - 1) "
                         f"for a {height} x {width} image")
    t = np.arange(-radius, radius + 1, dtype=np.float64)
    e = np.exp(-(t * t) / (2.0 * sigma * sigma))
    g = np.rint(32768.0 * e / e.sum()).astype(np.int64)
    g[radius] += 32768 - int(g.sum())
    return g.astype(np.int32)


def noise(height, width, seed_lo, seed_hi, comp):
    """n(y, x) of the specification: int64 [H, W] in [-32768, 32767]"""
    total = height * width
    ctr = np.arange((total + 7) >> 3, dtype=np.uint64)
    words = philox4x32(ctr & _LO, ctr >> _S32, comp, 0x5bd1e995, seed_lo, seed_hi)
    halves = np.empty((ctr.size, 8), dtype=np.int64)
    for j, w in enumerate(words):
        halves[:, 2 * j] = (w & np.uint64(0xFFFF)).astype(np.int64)
        halves[:, 2 * j + 1] = (w >> np.uint64(16)).astype(np.int64)
    return halves.reshape(-1)[:total].reshape(height, width) - 32768


def _blur_axis(a, g, axis):
    radius = (g.size - 1) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (radius, radius)
    ap = np.pad(a, pad, mode="reflect")            # reflect-101; a single fold because R <= extent - 1
    n = a.shape[axis]
    acc = np.zeros_like(a)
    tmp = np.empty_like(a)
    for k in range(g.size):
        sl = ap[:, k:k + n] if axis == 1 else ap[k:k + n, :]
        np.multiply(sl, int(g[k]), out=tmp)
        acc += tmp
    return acc


def field(height, width, taps, seed_lo, seed_hi, comp):
    """(h, v) of the specification for one component: int64 [H, W] each"""
    g = np.asarray(taps, dtype=np.int64)
    h = rs(_blur_axis(noise(height, width, seed_lo, seed_hi, comp), g, 1), 15)
    return h, _blur_axis(h, g, 0)


def _fold_clamp(q, lim):
    q = np.abs(q)
    q = np.where(q > lim, 2 * lim - q, q)
    return np.clip(q, 0, lim)


def _check_params(params, n_src):
    p = np.asarray(params)
    if p.ndim != 2 or p.shape[1] != ROW or p.dtype != np.int32:
        raise ValueError("augment: params must be int32 [n, 16]")
    if p.shape[0] == 0:
        raise ValueError("augment: no output images")
    if ((p[:, 0] < 0) | (p[:, 0] >= n_src)).any():
        raise ValueError(f"augment: source index outside [0, {n_src})")
    if ((p[:, 8] < 0) | (p[:, 8] > 256 * 256)).any():
        raise ValueError("augment: alpha outside [0, 256]")
    if (p[:, 1] & ~7).any() or p[:, 11:].any():
        raise ValueError("augment: reserved flag bits / row entries 11-15 must be zero")
    return p


def augment_host(src, params, sigma):
    """The specification, executable: src uint8 [n_src, H, W] (any strides), params int32 [n, 16] -> uint8 [n, 3, H, W]."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3:
        raise ValueError("augment: src must be uint8 [n_src, H, W]")
    n_src, H, W = src.shape
    if not (1 <= H <= MAX_EXTENT and 1 <= W <= MAX_EXTENT):
        raise ValueError(f"augment: extents outside [1, {MAX_EXTENT}]")
    params = _check_params(params, n_src)
    taps = gaussian_taps(sigma, H, W)
    out = np.empty((params.shape[0], 3, H, W), dtype=np.uint8)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    for r, row in enumerate(params.astype(np.int64)):
        idx, flags, m00, m01, m10, m11, b0, b1, alpha_q8, seed_lo, seed_hi = (int(v) for v in row[:11])
        qx, qy = xs << 16, ys << 16
        if flags & FLAG_ELASTIC:
            dx = rs(alpha_q8 * field(H, W, taps, seed_lo, seed_hi, 0)[1], 22)
            dy = rs(alpha_q8 * field(H, W, taps, seed_lo, seed_hi, 1)[1], 22)
            qx = _fold_clamp(qx + dx, (W - 1) << 16)
            qy = _fold_clamp(qy + dy, (H - 1) << 16)
        sx = rs(rs(m00 * qx + m01 * qy, 16) + b0, 8)
        sy = rs(rs(m10 * qx + m11 * qy, 16) + b1, 8)
        if flags & FLAG_HFLIP:
            sx = ((W - 1) << 8) - sx
        if flags & FLAG_VFLIP:
            sy = ((H - 1) << 8) - sy
        ix, fx, iy, fy = sx >> 8, sx & 255, sy >> 8, sy & 255
        img = src[idx]

        def tap(ty, tx):
            ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
            return np.where(ok, img[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)], 0).astype(np.int64)

        acc = ((256 - fx) * (256 - fy) * tap(iy, ix) + fx * (256 - fy) * tap(iy, ix + 1)
               + (256 - fx) * fy * tap(iy + 1, ix) + fx * fy * tap(iy + 1, ix + 1))
        out[r, :] = rs(acc, 16).astype(np.uint8)[None]
    return out


def augment(src, params, sigma, out=None):
    """uint8 [n, 3, H, W]: numpy arrays / CPU tensors take the host path (the specification), HIP tensors ``mc_augment_u8``.
    src: uint8 [n_src, H, W], any strides (e.g. ``hwc[..., 0]``); params: int32 [n, 16]."""
    import torch
    if torch.is_tensor(src) and src.is_cuda:
        from . import ops
        return ops.augment_u8(src, params, sigma, out=out)
    as_tensor = torch.is_tensor(src)
    res = augment_host(src.numpy() if as_tensor else src, params.numpy() if torch.is_tensor(params) else params, sigma)
    if out is not None:
        if tuple(out.shape) != res.shape or str(out.dtype).split(".")[-1] != "uint8":
            raise ValueError("augment: out must be uint8 [n, 3, H, W]")
        out[...] = torch.from_numpy(res) if torch.is_tensor(out) else res
        return out
    return torch.from_numpy(res) if as_tensor else res


def identity_rows(n, src_index=None):
    p = np.zeros((n, ROW), dtype=np.int32)
    p[:, 0] = np.arange(n) if src_index is None else src_index
    p[:, 2] = p[:, 5] = 65536
    return p


class AugmentPolicy:
    """The reference's train transform as a sampler of parameter rows.  Distributions (stated, not pinned to the library):
    with probability ``p`` a sample is transformed at all, else its row is the identity; within a transformed sample each of
    horizontal flip, vertical flip, affine and elastic is applied with probability 0.5 (the library's per-transform default);
    rotation and shear (along x) uniform in +-degrees, translation uniform in +-percent of the extent per axis, scale uniform
    in its range per axis.  The forward matrix T(centre) T(translate) R(rotate) Sh(shear) S(scale) T(-centre), centre
    ((W-1)/2, (H-1)/2), is inverted in fp64 and quantised to Q16."""

    def __init__(self, degree=20.0, translate_percent=0.1, scale=(0.8, 1.2), shear=20.0, alpha=10.0, sigma=15.0, p=1.0,
                 size=(1520, 912)):
        self.size = (int(size[0]), int(size[1]))          # (H, W) that ``sample`` quantises translations and centres for
        self.degree, self.translate_percent, self.shear = float(degree), float(translate_percent), float(shear)
        self.scale = (float(scale[0]), float(scale[1])) if isinstance(scale, (tuple, list)) else (float(scale), float(scale))
        self.alpha, self.sigma, self.p = float(alpha), float(sigma), float(p)
        if not 0.0 <= self.alpha <= 256.0:
            raise ValueError("AugmentPolicy: alpha outside [0, 256]")
        if not self.sigma >= 0.5:
            raise ValueError("AugmentPolicy: sigma must be >= 0.5")

    @classmethod
    def from_transform_config(cls, cfg, size=(1520, 912)):
        """cfg: the ``train.transform`` mapping of the reference's configs/transform/clahe.yaml (or the whole file's dict);
        size: (H, W) of the images, the reference's 1520 x 912 by default"""
        cfg = cfg.get("train", cfg)
        cfg = cfg.get("transform", cfg)
        return cls(degree=cfg["affine_transform_degree"], translate_percent=cfg["affine_translate_percent"],
                   scale=tuple(cfg["affine_scale"]), shear=cfg["affine_shear"], alpha=cfg["elastic_transform_alpha"],
                   sigma=cfg["elastic_transform_sigma"], p=cfg["p"], size=size)

    def draw(self, n, generator):
        """the random draws behind ``sample``: a dict of [n] arrays (fp64 / bool / uint32)"""
        import torch
        u = torch.rand((n, 11), generator=generator, dtype=torch.float64).numpy()
        seeds = torch.randint(0, 1 << 32, (n, 2), generator=generator, dtype=torch.int64).numpy().astype(np.uint32)
        on = u[:, 0] < self.p
        sym = lambda c, a: (2.0 * u[:, c] - 1.0) * a   # noqa: E731
        return {"hflip": on & (u[:, 1] < 0.5), "vflip": on & (u[:, 2] < 0.5), "affine": on & (u[:, 3] < 0.5),
                "elastic": on & (u[:, 4] < 0.5), "rotate": sym(5, self.degree), "shear": sym(6, self.shear),
                "translate_x": sym(7, self.translate_percent), "translate_y": sym(8, self.translate_percent),
                "scale_x": self.scale[0] + u[:, 9] * (self.scale[1] - self.scale[0]),
                "scale_y": self.scale[0] + u[:, 10] * (self.scale[1] - self.scale[0]),
                "seed_lo": seeds[:, 0], "seed_hi": seeds[:, 1]}

    def rows(self, draws, height, width, src_index=None):
        n = len(draws["rotate"])
        p = identity_rows(n, src_index)
        p[:, 1] = (draws["hflip"] * FLAG_HFLIP + draws["vflip"] * FLAG_VFLIP + draws["elastic"] * FLAG_ELASTIC)
        for i in np.nonzero(draws["affine"])[0]:
            inv = np.linalg.inv(affine_matrix(draws["rotate"][i], draws["shear"][i], draws["scale_x"][i], draws["scale_y"][i],
                                              draws["translate_x"][i] * width, draws["translate_y"][i] * height, height, width))
            p[i, 2:6] = np.rint(inv[:2, :2] * 65536.0).reshape(-1)
            p[i, 6:8] = np.rint(inv[:2, 2] * 65536.0)
        p[:, 8] = np.where(draws["elastic"], int(round(self.alpha * 256.0)), 0)
        p[:, 9] = draws["seed_lo"].view(np.int32)
        p[:, 10] = draws["seed_hi"].view(np.int32)
        return p

    def sample(self, n, generator, size=None, src_index=None):
        """int32 [n, 16] rows for images of ``size`` = (H, W) (default: the policy's) from a ``torch.Generator``; every row
        gets a fresh 64-bit seed"""
        size = self.size if size is None else size
        return self.rows(self.draw(n, generator), int(size[0]), int(size[1]), src_index)


def affine_matrix(rotate_deg, shear_deg, scale_x, scale_y, tx, ty, height, width):
    """forward 3x3 matrix (source -> output pixel coordinates) about the image centre, fp64"""
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    a, s = math.radians(rotate_deg), math.tan(math.radians(shear_deg))
    rot = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    shr = np.array([[1.0, s, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    scl = np.diag([scale_x, scale_y, 1.0])
    to_c = np.array([[1.0, 0.0, -cx], [0.0, 1.0, -cy], [0.0, 0.0, 1.0]])
    back = np.array([[1.0, 0.0, cx + tx], [0.0, 1.0, cy + ty], [0.0, 0.0, 1.0]])
    return back @ rot @ shr @ scl @ to_c


def make_views(src, policy, generator, mean, std, src_view=None):
    """{"images": RawImages, "image_views": RawImages} for ``BreastClip.forward``: two independently sampled augmentations
    per pair, both written by ONE launch sequence (n_out = 2b).  src: uint8 [b, H, W] on the HIP device; the second view comes
    from ``src_view`` (the other image of the study [ref: imagetext.py:137-150]) where given, else from ``src`` too."""
    import torch
    from . import ops
    b, H, W = src.shape
    if src_view is not None:
        if src_view.shape != src.shape or src_view.device != src.device or src_view.dtype != src.dtype:
            raise ValueError("make_views: src_view must match src")
        planes = torch.cat([src, src_view], 0)
    else:
        planes = src
    first = policy.sample(b, generator, (H, W), np.arange(b))
    second = policy.sample(b, generator, (H, W), np.arange(b) + (b if src_view is not None else 0))
    out = augment(planes, np.concatenate([first, second], 0), policy.sigma)
    return {"images": ops.RawImages(out[:b], mean, std), "image_views": ops.RawImages(out[b:], mean, std)}
