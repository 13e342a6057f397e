"""mc_augment_u8 on the device against the host path of mammo_clip_amd/augment.py (the integer specification): every byte
equal, no tolerance.  Odd extents that are no multiple of any tile, R equal to the extent minus one, the smallest R, a
strided source, alpha at its cap, workspace chunking, a second stream, and the production shape."""
import types

import numpy as np
import pytest
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import augment as A
from mammo_clip_amd import lib as L
from mammo_clip_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

#        H    W   sigma  source layout  alpha of the elastic-only row
CASES = [(61, 61, 15.0, "planes", 120.0),        # R = 60 = W - 1 = H - 1
         (130, 97, 3.0, "hwc", 120.0),           # sw = 3: the source is a channel of an HWC array
         (200, 333, 6.5, "planes", 256.0),       # alpha at the cap; 4 x 6 tiles
         (67, 45, 0.5, "planes", 120.0),         # the smallest R (2)
         (35, 1100, 2.0, "planes", 120.0)]       # wider than one row segment of the horizontal pass (1024 outputs)


def _rows(H, W, alpha_el):
    """identity, flips only, affine only, elastic only, everything on; rows 1 and 4 read the same source"""
    fwd = A.affine_matrix(17.0, -12.0, 0.85, 1.15, 0.07 * W, -0.05 * H, H, W)
    inv = np.linalg.inv(fwd)
    m = [int(v) for v in np.rint(inv[:2, :2] * 65536).reshape(-1)]
    b = [int(v) for v in np.rint(inv[:2, 2] * 65536)]
    ident = [65536, 0, 0, 65536, 0, 0]
    rows = [[0, 0, *ident, 0, 0, 0],
            [1, 3, *ident, 0, 0, 0],
            [2, 0, *m, *b, 0, 0, 0],
            [0, 4, *ident, int(alpha_el * 256), 0x9e3779b9 - (1 << 32), 0x7f4a7c15],
            [1, 7, *m, *b, 10 * 256, 12345, -67890]]
    return np.asarray([r + [0] * 5 for r in rows], dtype=np.int32)


_CACHE = {}


def _case(i):
    """(device source planes, rows, sigma, host result): built once per case and shared, never modified"""
    if i not in _CACHE:
        H, W, sigma, layout, alpha_el = CASES[i]
        rng = np.random.default_rng(100 + i)
        if layout == "hwc":
            hwc = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
            host_src, dev_src = hwc[..., 1], torch.from_numpy(hwc).to(DEV)[..., 1]
            assert dev_src.stride() == (H * W * 3, W * 3, 3)
        else:
            host_src = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
            dev_src = torch.from_numpy(host_src).to(DEV)
        rows = _rows(H, W, alpha_el)
        _CACHE[i] = (dev_src, rows, sigma, A.augment(host_src, rows, sigma))
    return _CACHE[i]


def _report(got, want, tag):
    got = got.cpu().numpy()
    bad = got != want
    per_row = bad.reshape(bad.shape[0], -1).sum(1).tolist()
    print(f"{tag}: differing bytes per row {per_row}, max |diff| {int(np.abs(got.astype(int) - want.astype(int)).max())}")
    return not bad.any()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_device_equals_host_every_byte(i):
    src, rows, sigma, want = _case(i)
    got = A.augment(src, rows, sigma)
    assert got.shape == want.shape and got.dtype == torch.uint8 and got.is_cuda
    assert _report(got, want, f"case {CASES[i][:3]}")
    # the elastic rows moved something, the affine row exposed the zero border
    assert (want[3] != want[0]).mean() > 0.2 and (want[2] == 0).mean() > 0.02


def test_result_does_not_depend_on_workspace_stream_or_repeat():
    src, rows, sigma, want = _case(1)
    H, W = want.shape[2:]
    one = L.load().mc_augment_ws_bytes(1, H, W)
    assert L.load().mc_augment_ws_bytes(5, H, W) == 5 * one
    small = ops.augment_u8(src, rows, sigma, ws_bytes=one)                     # five chunks of one image
    mid = ops.augment_u8(src, rows, sigma, ws_bytes=2 * one + 7)               # chunks of 2, 2, 1
    large = ops.augment_u8(src, rows, sigma, ws_bytes=64 * one)
    out = torch.empty_like(large)
    again = A.augment(src, rows, sigma, out=out)
    assert again is out
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other = A.augment(src, rows, sigma)
    st.synchronize()
    for tag, t in (("minimal ws", small), ("ws of 2.x images", mid), ("large ws", large), ("repeat", out), ("second stream", other)):
        assert _report(t, want, tag), tag
    with pytest.raises(L.MammoClipHipError):
        ops.augment_u8(src, rows, sigma, ws_bytes=one - 1)
    bad = rows.copy()
    bad[2, 0] = 3
    with pytest.raises(ValueError):
        ops.augment_u8(src, bad, sigma)


def test_production_shape_against_host():
    """two rows from one 1520 x 912 source at alpha 10, sigma 15: the 64-bit products of the map and i >> 3 past 2^20"""
    H, W = 1520, 912
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(5)
    img = ((np.sin(x / 37.0) * np.cos(y / 51.0) * 100 + 128).astype(np.int64) + rng.integers(-20, 21, (H, W))).clip(0, 255)
    src = img.astype(np.uint8)[None]
    pol = A.AugmentPolicy.from_transform_config({"affine_transform_degree": 20, "affine_translate_percent": 0.1,
                                                 "affine_scale": [0.8, 1.2], "affine_shear": 20, "elastic_transform_alpha": 10,
                                                 "elastic_transform_sigma": 15, "p": 1.0})
    d = pol.draw(2, torch.Generator().manual_seed(11))
    for k in ("affine", "elastic"):
        d[k][:] = True
    d["hflip"][:], d["vflip"][:] = [True, False], [False, True]
    rows = pol.rows(d, H, W, np.zeros(2, dtype=np.int64))
    assert (rows[:, 8] == 2560).all() and (rows[:, 1] & 4).all()
    got = A.augment(torch.from_numpy(src).to(DEV), rows, pol.sigma)
    want = A.augment(src, rows, pol.sigma)
    assert _report(got, want, "1520 x 912")


def test_make_views_feeds_the_model_like_the_host_bytes():
    """make_views -> BreastClip.forward (small B2 model, eval mode): the loss equals, bit for bit, the loss of a batch whose
    RawImages hold the host path's bytes for the same rows"""
    from mammo_clip_amd.breastclip import util
    from mammo_clip_amd.breastclip.loss import build_loss
    from mammo_clip_amd.breastclip.model import build_model
    from oracle import arch as oarch, bert as obert, weights as ow

    cfg = {"name": "clip_custom", "temperature": 0.07,
           "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
           "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                            "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
           "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
    loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
    torch.cuda.set_device(DEV)
    util.GlobalEnv.reset()
    model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996))
    arch = oarch.build_arch("efficientnet-b2")
    model.load_state_dict(ow.synth_state_dict(ow.clip_shapes(arch, obert.BertShape()), seed=10), strict=True)
    model = model.to(DEV).eval()
    lossf = build_loss(loss_cfg)
    b, H, W, T = 2, 64, 64, 16
    batch = ow.synth_batch(b, H, W, T, seed=3)
    text = {k: {kk: v.to(DEV) for kk, v in batch[k].items()} for k in ("text_tokens", "text_tokens2")}
    rng = np.random.default_rng(9)
    src, src_view = (rng.integers(0, 256, (b, H, W), dtype=np.uint8) for _ in range(2))
    pol = A.AugmentPolicy(sigma=3.0, alpha=40.0, size=(H, W))
    mean, std = 0.3089279, 0.25053555408335154

    for view in (None, src_view):
        g = torch.Generator().manual_seed(21)
        state = g.get_state()
        views = A.make_views(torch.from_numpy(src).to(DEV), pol, g, mean, std,
                             src_view=None if view is None else torch.from_numpy(view).to(DEV))
        assert isinstance(views["images"], ops.RawImages) and views["images"].shape == (b, 3, H, W)
        # the same rows on the host
        g.set_state(state)
        first = pol.sample(b, g, (H, W), np.arange(b))
        second = pol.sample(b, g, (H, W), np.arange(b) + (0 if view is None else b))
        planes = src if view is None else np.concatenate([src, view], 0)
        host = A.augment(planes, np.concatenate([first, second], 0), pol.sigma)
        assert not np.array_equal(host[:b], host[b:])
        losses = []
        for imgs, vws in ((views["images"], views["image_views"]),
                          (ops.RawImages(torch.from_numpy(host[:b]).to(DEV), mean, std),
                           ops.RawImages(torch.from_numpy(host[b:]).to(DEV), mean, std))):
            util.GlobalEnv.reset()
            with torch.no_grad():
                out = model({"images": imgs, "image_views": vws, **text}, DEV)
                losses.append(float(lossf(**out, is_train=False)["total"]))
        print(f"make_views (src_view {'given' if view is not None else 'absent'}): loss {losses[0]!r} vs host bytes {losses[1]!r}")
        assert np.isfinite(losses[0]) and losses[0] == losses[1]
