"""The MLP projection head without a device: construction and state-dict layout, the fp64 yardstick of the GPU tests against
the reference-generated golden file, the host Philox mask, and the argument validation of the new entry points (every check
fires before a launch, so host pointers do)."""
import types

import numpy as np
import pytest
import torch

import mammo_clip_amd  # noqa: F401
import mammo_clip_amd.lib as L
from mammo_clip_amd.breastclip.model import build_model
from mammo_clip_amd.breastclip.model.modules import LinearProjectionHead, MLPProjectionHead, load_projection_head
import _mlp_head_common as H

HEAD_KEYS = ["projection.weight", "projection.bias", "fc.weight", "fc.bias", "layer_norm.weight", "layer_norm.bias"]


def test_load_projection_head_mlp_builds_the_reference_module_layout():
    head = load_projection_head(40, {"name": "mlp", "dropout": 0.1, "proj_dim": 24})
    assert isinstance(head, MLPProjectionHead)
    assert [(k, tuple(v.shape)) for k, v in head.named_parameters()] == [
        ("projection.weight", (24, 40)), ("projection.bias", (24,)), ("fc.weight", (24, 24)), ("fc.bias", (24,)),
        ("layer_norm.weight", (24,)), ("layer_norm.bias", (24,))]
    assert list(head.state_dict()) == HEAD_KEYS
    assert isinstance(head.projection, torch.nn.Linear) and isinstance(head.fc, torch.nn.Linear)
    assert isinstance(head.layer_norm, torch.nn.LayerNorm) and head.layer_norm.eps == 1e-5
    assert isinstance(head.dropout, torch.nn.Dropout) and head.dropout.p == 0.1
    # nn.LayerNorm's default initialisation
    assert torch.equal(head.layer_norm.weight, torch.ones(24)) and torch.equal(head.layer_norm.bias, torch.zeros(24))
    assert isinstance(load_projection_head(40, {"name": "linear", "dropout": 0.1, "proj_dim": 24}), LinearProjectionHead)


def test_breastclip_with_mlp_heads_has_the_reference_state_dict_keys():
    tok = types.SimpleNamespace(vocab_size=28996)
    loss_cfg = H.LOSS_CFG
    lin = list(build_model(H.cfg("linear"), loss_cfg, tok).state_dict())
    model = build_model(H.cfg("mlp"), loss_cfg, tok)
    keys = list(model.state_dict())
    expect = []
    for k in lin:                                   # module order: each head's two linear keys become its six
        if k.endswith("_projection.projection.weight"):
            expect += [k[:-len("projection.weight")] + s for s in HEAD_KEYS]
        elif not k.endswith("_projection.projection.bias"):
            expect.append(k)
    assert keys == expect and len(keys) == len(lin) + 8
    assert set(keys) - set(lin) == {f"{h}_projection.{s}" for h in ("image", "text") for s in HEAD_KEYS[2:]}
    sd = H.mlp_state_dict()
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model.text_projection.layer_norm.weight, sd["text_projection.layer_norm.weight"])
    assert model.image_projection.projection.weight.shape == (512, 1408)
    assert model.text_projection.projection.weight.shape == (512, 768)


def test_fp64_restatement_reproduces_the_reference_golden():
    x, w, cot, out, grads = H.load_golden()
    assert x.shape == (5, 40) and out.shape == (5, 24) and x.dtype == torch.float64
    assert float((w["layer_norm.weight"] - 1).abs().max()) > 0.1 and float(w["layer_norm.bias"].abs().max()) > 0.1
    got, g = H.head64_grads(x, w, cot, 1.0)
    assert float((got - out).abs().max()) <= 1e-13 * float(out.abs().max())
    assert set(g) == set(grads) == set(H.PARAMS) | {"x"}
    for k in grads:
        assert float((g[k] - grads[k]).abs().max()) <= 1e-12 * float(grads[k].abs().max()), k


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_host_mask_keep_rate_inside_the_binomial_band(p):
    rows, n = 128, 512                              # 2^16 elements
    keep = H.keep_mask(rows, n, p, 0x9E3779B97F4A7C15, 3)
    assert keep.shape == (rows, n) and keep.dtype == bool
    q = 1.0 - int(np.float32(p) * np.float32(65536.0)) / 65536.0      # the keep probability of the 16-bit threshold
    N = rows * n
    assert abs(int(keep.sum()) - N * q) <= 6.0 * (N * q * (1.0 - q)) ** 0.5
    assert not np.array_equal(keep, H.keep_mask(rows, n, p, 0x9E3779B97F4A7C15, 4))        # the stream id matters
    assert not np.array_equal(keep, H.keep_mask(rows, n, p, 0x1E3779B97F4A7C15, 3))        # ... and the high seed word
    assert H.keep_mask(3, 8, 0.0, 1, 1).all()


def _err():
    return L.load().mc_last_error().decode()


def test_entry_points_validate_before_any_launch():
    lib = L.load()
    assert lib.mc_mlp_head_max_n() >= 1024 and lib.mc_mlp_head_max_n() == MLPProjectionHead.max_projection_dim
    nmax = lib.mc_mlp_head_max_n()
    for n, ok in ((8, 1), (512, 1), (520, 1), (nmax, 1), (12, 0), (0, 0), (-8, 0), (4, 0), (nmax + 8, 0)):
        assert lib.mc_mlp_head_supported(n) == ok, n
    assert lib.mc_mlp_head_ln_bwd_ws_rows(1) == 1 and lib.mc_mlp_head_ln_bwd_ws_rows(5) == 2
    cap = lib.mc_mlp_head_ln_bwd_ws_rows(1 << 20)
    assert lib.mc_mlp_head_ln_bwd_ws_rows(4 * cap) == cap and lib.mc_mlp_head_ln_bwd_ws_rows(4 * cap + 1) == cap
    buf = np.zeros(64, dtype=np.float32)            # a host buffer: never dereferenced, every call below is refused
    a = buf.ctypes.data

    def fwd(f=a, rows=4, n=8, p=0.1):
        return lib.mc_mlp_head_ln_fwd(f, a, a, a, 1e-5, rows, n, p, 1, 0, a, a, a, None)

    def bwd(dy=a, rows=5, n=8, p=0.1, ws_rows=2):
        return lib.mc_mlp_head_ln_bwd(dy, a, a, a, rows, n, p, 1, 0, a, a, a, ws_rows, None)

    for call, name in ((fwd, "mlp_head_ln_fwd"), (bwd, "mlp_head_ln_bwd")):
        for kw in (dict(n=12), dict(n=0), dict(n=nmax + 8), dict(rows=0), dict(p=1.0), dict(p=-0.5)):
            assert call(**kw) != 0 and name in _err(), (name, kw, _err())
    assert fwd(f=None) != 0 and "mlp_head_ln_fwd" in _err() and "null" in _err()
    assert bwd(dy=None) != 0 and "mlp_head_ln_bwd" in _err() and "null" in _err()
    assert bwd(ws_rows=3) != 0 and "mlp_head_ln_bwd" in _err() and "ws_rows" in _err()
    assert bwd(ws_rows=0) != 0 and "ws_rows" in _err()
    assert lib.mc_gelu_f32_fwd(None, a, 8, None) != 0 and "gelu_f32_fwd" in _err()
    assert lib.mc_gelu_f32_fwd(a, a, 0, None) != 0 and "gelu_f32_fwd" in _err()
    assert lib.mc_gelu_f32_bwd_add(a, a, None, a, 8, None) != 0 and "gelu_f32_bwd_add" in _err()
    assert lib.mc_gelu_f32_bwd_add(a, a, a, a, -1, None) != 0 and "gelu_f32_bwd_add" in _err()


def test_module_rejects_unsupported_widths_and_cpu_input():
    for n in (12, 0, MLPProjectionHead.max_projection_dim + 8):
        with pytest.raises(ValueError, match=str(MLPProjectionHead.max_projection_dim)):
            MLPProjectionHead(40, n, 0.1)
    with pytest.raises(ValueError):
        load_projection_head(40, {"name": "mlp", "dropout": 0.1, "proj_dim": 12})
    head = MLPProjectionHead(40, 24, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(torch.zeros(2, 40))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LinearProjectionHead(40, 24)(torch.zeros(2, 40))


def test_new_operators_are_registered_with_fake_implementations():
    import mammo_clip_amd.custom_ops as co
    for name in ("gelu_f32", "gelu_f32_bwd_add", "mlp_head_ln", "mlp_head_ln_bwd"):
        assert name in co.OPS and hasattr(torch.ops.mammoclip, name)
    f = torch.empty(5, 24, device="meta")
    v = torch.empty(24, device="meta")
    y, xhat, rstd = torch.ops.mammoclip.mlp_head_ln(f, f, v, v, 1e-5, 0.1, 7, 1)
    assert y.shape == xhat.shape == (5, 24) and rstd.shape == (5,)
    outs = torch.ops.mammoclip.mlp_head_ln_bwd(f, f, rstd, v, 0.1, 7, 1)
    assert [tuple(o.shape) for o in outs] == [(5, 24), (5, 24), (24,), (24,), (24,)]
    assert torch.ops.mammoclip.gelu_f32_bwd_add(f, f, f).shape == (5, 24)
