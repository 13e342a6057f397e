"""Long fused attention (mc_attn_long_* / mc_attn_varlen_long_*, 257..512 keys), the host side: the C ABI of the six new
entries, their shape predicates and argument checks, and which kernel a text-encoder layer picks for a given T.  No HIP kernel
is launched here (`pytest -m "not gpu"`)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import lib as L, ops  # noqa: E402
from mammo_clip_amd.breastclip.model.modules import text_encoder as te  # noqa: E402

P, I, F, LL, ULL, U = L.P, L.I, L.F, L.LL, L.ULL, L.U
NEW_ENTRIES = {
    "mc_attn_long_supported": ([I, I], I),
    "mc_attn_long_fwd": ([P, P, I, I, I, F, F, ULL, U, P, P, P], I),
    "mc_attn_long_bwd": ([P, P, P, P, I, I, I, F, F, ULL, U, P, P], I),
    "mc_attn_varlen_long_supported": ([I, I], I),
    "mc_attn_varlen_long_fwd": ([P, P, P, I, I, I, LL, I, F, F, ULL, U, P, P, P], I),
    "mc_attn_varlen_long_bwd": ([P, P, P, P, P, I, I, I, LL, I, F, F, ULL, U, P, P], I),
}
_CTYPE = {"void*": P, "float*": P, "mc_bf16*": P, "int*": P, "int": I, "float": F, "long long": LL, "unsigned long long": ULL,
          "unsigned int": U}


def test_header_library_and_binding_agree_on_the_new_entries():
    """declared in the header, exported by both storage builds, bound in lib.py with the header's argument list"""
    header = open(os.path.join(ROOT, "include", "mammoclip_hip.h")).read()
    lib = L.load()
    f16 = ctypes.CDLL(os.path.join(os.path.dirname(L.LIB_PATH), "libmammoclip_hip_f16.so"))
    for name, (args, res) in NEW_ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, name + " is not declared in the header"
        decl = []
        for prm in m.group(1).split(","):
            ty = re.sub(r"\bconst\b", "", prm).strip()
            ty = re.sub(r"\s*\b[a-z_0-9]+$", "", ty).replace(" *", "*").strip()           # drop the parameter name
            decl.append(_CTYPE[ty])
        assert decl == args, (name, decl, args)
        assert L._SIGS[name] == (args, res), name
        assert name in L.EXPORTS and hasattr(lib, name) and hasattr(f16, name), name
    # the resident entries and their signatures stay; the long entries take the same arguments
    assert L._SIGS["mc_attn_bwd"] == ([P, P, P, P, I, I, I, F, F, ULL, U, P, P], I)
    assert L._SIGS["mc_attn_varlen_bwd"] == ([P, P, P, P, P, I, I, I, LL, I, F, F, ULL, U, P, P], I)


@pytest.mark.parametrize("t,hd,ok", [(32, 64, True), (256, 64, True), (288, 64, True), (512, 64, True),
                                     (544, 64, False), (300, 64, False), (512, 32, False)])
def test_long_predicate(t, hd, ok, monkeypatch):
    monkeypatch.delenv("MC_FUSED_ATTN", raising=False)
    assert bool(L.load().mc_attn_long_supported(t, hd)) is ok and ops.attn_long_supported(t, hd) is ok


@pytest.mark.parametrize("n,hd,ok", [(1, 64, True), (257, 64, True), (512, 64, True),
                                     (0, 64, False), (513, 64, False), (64, 32, False)])
def test_varlen_long_predicate(n, hd, ok):
    assert bool(L.load().mc_attn_varlen_long_supported(n, hd)) is ok and ops.attn_varlen_long_supported(n, hd) is ok


def test_resident_predicates_are_unchanged(monkeypatch):
    monkeypatch.delenv("MC_FUSED_ATTN", raising=False)
    lib = L.load()
    assert not lib.mc_attn_supported(512, 64) and not lib.mc_attn_varlen_supported(257, 64)
    assert lib.mc_attn_supported(256, 64) and lib.mc_attn_varlen_supported(256, 64)
    assert not ops.attn_supported(512, 64) and not ops.attn_varlen_supported(257, 64)


def test_new_entries_validate_their_arguments_without_a_launch():
    """null pointers, t = 544, max_len = 513 and p = 1.0: a status and an error string, before any launch (the non-null
    pointers below are never dereferenced by a call that fails its checks)"""
    lib = L.load()
    x = 16
    # null pointers
    assert lib.mc_attn_long_fwd(None, x, 1, 512, 1, 0.125, 0.0, 1, 0, x, x, None) != 0 and b"attn_long_fwd" in lib.mc_last_error()
    assert lib.mc_attn_long_bwd(x, x, x, None, 1, 512, 1, 0.125, 0.0, 1, 0, x, None) != 0
    assert b"attn_long_bwd" in lib.mc_last_error()
    assert lib.mc_attn_varlen_long_fwd(x, None, None, 1, 512, 512, 512, 1, 0.125, 0.0, 1, 0, x, x, None) != 0
    assert b"attn_varlen_long_fwd" in lib.mc_last_error()
    assert lib.mc_attn_varlen_long_bwd(x, x, None, x, None, 1, 512, 512, 512, 1, 0.125, 0.0, 1, 0, x, None) != 0
    assert b"attn_varlen_long_bwd" in lib.mc_last_error()
    # shapes
    for t in (544, 300, 0):
        assert lib.mc_attn_long_fwd(x, x, 1, t, 1, 0.125, 0.0, 1, 0, x, x, None) != 0 and b"attn_long" in lib.mc_last_error()
        assert lib.mc_attn_long_bwd(x, x, x, x, 1, t, 1, 0.125, 0.0, 1, 0, x, None) != 0 and b"attn_long" in lib.mc_last_error()
    for n in (513, 0):
        assert lib.mc_attn_varlen_long_fwd(x, x, None, 1, n, 520, 520, 1, 0.125, 0.0, 1, 0, x, x, None) != 0
        assert b"attn_varlen_long" in lib.mc_last_error()
        assert lib.mc_attn_varlen_long_bwd(x, x, None, x, x, 1, n, 520, 520, 1, 0.125, 0.0, 1, 0, x, None) != 0
        assert b"attn_varlen_long" in lib.mc_last_error()
    # dropout probability
    assert lib.mc_attn_long_fwd(x, x, 1, 512, 1, 0.125, 1.0, 1, 0, x, x, None) != 0 and b"dropout" in lib.mc_last_error()
    assert lib.mc_attn_long_bwd(x, x, x, x, 1, 512, 1, 0.125, 1.0, 1, 0, x, None) != 0 and b"dropout" in lib.mc_last_error()
    assert lib.mc_attn_varlen_long_fwd(x, x, None, 1, 512, 512, 512, 1, 0.125, 1.0, 1, 0, x, x, None) != 0
    assert b"dropout" in lib.mc_last_error()
    assert lib.mc_attn_varlen_long_bwd(x, x, None, x, x, 1, 512, 512, 512, 1, 0.125, 1.0, 1, 0, x, None) != 0
    assert b"dropout" in lib.mc_last_error()


# ------------------------------------------------------------------------------------------------ routing
class _Routed(Exception):
    pass


@pytest.fixture()
def layer(monkeypatch):
    """one BertLayer on the host whose kernels are stubs: the QKV projection returns zeros, and the first attention kernel a
    call reaches (any of the six wrappers, or the unfused path's first GEMM) ends the call with its name"""
    monkeypatch.delenv("MC_FUSED_ATTN", raising=False)
    model = te.BertModelHIP(te.BertConfigLite(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=256,
                                              vocab_size=64))
    monkeypatch.setattr(ops, "cast_bf16", lambda w, out=None: out if out is not None else w.detach().to(ops.BF16))
    monkeypatch.setattr(ops, "linear_fwd", lambda inp, w, bias=None, residual=None: torch.zeros((inp.shape[0], w.shape[0]), dtype=ops.BF16))

    def stop(name):
        def f(*a, **kw):
            raise _Routed(name)
        return f
    for name in ("attn_fwd", "attn_long_fwd", "attn_varlen_fwd", "attn_varlen_long_fwd", "gemm"):
        monkeypatch.setattr(ops, name, stop(name))
    return model.encoder.layer[0]


def _route(lyr, t=None, lengths=None):
    if lengths is None:
        b, pk, x = 2, None, torch.zeros((2 * t, 128), dtype=ops.BF16)
    else:
        pk = ops.PackedRows(lengths, 512)
        b, t, x = pk.b, pk.t, torch.zeros((pk.rows, 128), dtype=ops.BF16)
    with pytest.raises(_Routed) as e:
        te._LayerFn.forward(None, x, None, lyr, b, t, 1, pk)
    return str(e.value)


def test_padded_routing(layer, monkeypatch):
    assert _route(layer, t=256) == "attn_fwd" and _route(layer, t=32) == "attn_fwd"
    assert _route(layer, t=288) == "attn_long_fwd" and _route(layer, t=512) == "attn_long_fwd"
    assert _route(layer, t=264) == "gemm" and _route(layer, t=544) == "gemm"       # neither: the unfused GEMMs
    monkeypatch.setenv("MC_FUSED_ATTN", "0")
    assert [_route(layer, t=t) for t in (256, 288, 512)] == ["gemm"] * 3


def test_packed_routing(layer):
    assert _route(layer, lengths=[256, 5]) == "attn_varlen_fwd"
    assert _route(layer, lengths=[257, 5]) == "attn_varlen_long_fwd" and _route(layer, lengths=[512, 1]) == "attn_varlen_long_fwd"


def test_packed_head_size_other_than_64_still_raises(layer):
    layer.heads = 4                                    # head size 32
    pk = ops.PackedRows([300, 5], 512)
    with pytest.raises(RuntimeError, match="no variable-length attention kernel"):
        te._LayerFn.forward(None, torch.zeros((pk.rows, 128), dtype=ops.BF16), None, layer, pk.b, pk.t, 1, pk)
