"""Frozen BatchNorm (EfficientNet.freeze_bn / backward in eval mode), the host side: the public switch, the state_dict, the C ABI
of the new entries and MBConvBlock.plan in frozen mode.  No HIP kernel is launched here (`pytest -m "not gpu"`)."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import lib as L  # noqa: E402
from mammo_clip_amd.breastclip.model import build_model  # noqa: E402
from mammo_clip_amd.breastclip.model.modules.efficientnet_custom import EfficientNet  # noqa: E402

NEW_ENTRIES = {
    "mc_bn_eval_stats": ([L.P, L.P, L.P, L.P, L.F, L.I, L.P, L.P, L.P, L.P, L.P], L.I),
    "mc_bnact_bwd_frozen": ([ctypes.POINTER(L.BnactArgs), L.P], L.I),
    "mc_bn_bwd_finalize_frozen": ([L.P, L.I, L.I, L.P, L.P, L.P, L.P, L.P], L.I),
    "mc_bn_frozen_rows": ([L.P, L.P, L.I, L.I, L.P, L.P, L.P], L.I),
}
_CTYPE = {"void*": L.P, "float*": L.P, "mc_bf16*": L.P, "mc_bnact_args*": ctypes.POINTER(L.BnactArgs), "int": L.I, "float": L.F,
          "double": L.D, "long long": L.LL}


def _cfg():
    return {"name": "clip_custom", "temperature": 0.07,
            "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": True, "model_type": "cnn"},
            "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                             "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
            "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}


def test_switch_semantics_across_train_and_eval():
    """a BatchNorm site uses batch statistics iff training and not frozen_bn; the flag survives train() / eval(), reaches every
    block, is read-only as a property and freeze_bn returns self"""
    enc = EfficientNet.from_name("efficientnet-b2")
    assert enc.training and enc.frozen_bn is False and enc.batch_stats
    assert enc.freeze_bn() is enc and enc.frozen_bn is True and not enc.batch_stats
    assert all(b.frozen_bn and not b.batch_stats and b.training for b in enc._blocks)
    enc.eval()
    assert enc.frozen_bn and not enc.batch_stats and not any(b.batch_stats for b in enc._blocks)
    enc.train()
    assert enc.frozen_bn and not enc.batch_stats and all(b.training for b in enc._blocks)
    assert enc.freeze_bn(False) is enc and not enc.frozen_bn and enc.batch_stats and all(b.batch_stats for b in enc._blocks)
    enc.eval()
    assert not enc.frozen_bn and not enc.batch_stats           # eval alone: running statistics, flag off
    with pytest.raises(AttributeError):
        enc.frozen_bn = True


def test_fp8_with_frozen_statistics_is_refused():
    enc = EfficientNet.from_name("efficientnet-b2").freeze_bn()
    with pytest.raises(NotImplementedError, match="fp8"):
        enc.set_fp8(True)
    enc.freeze_bn(False).set_fp8(True)
    with pytest.raises(NotImplementedError, match="fp8"):
        enc.freeze_bn()
    assert not enc.frozen_bn and enc.fp8


def test_state_dict_is_unchanged_and_clip_passes_the_switch_through():
    model = build_model(_cfg(), {"breast_clip": {}}, types.SimpleNamespace(vocab_size=28996))
    keys = list(model.state_dict().keys())
    assert model.frozen_bn is False
    assert model.freeze_bn() is model and model.frozen_bn and model.image_encoder.frozen_bn
    sd = model.state_dict()
    assert list(sd.keys()) == keys and not any("frozen" in k for k in keys)
    fresh = build_model(_cfg(), {"breast_clip": {}}, types.SimpleNamespace(vocab_size=28996))
    ret = fresh.load_state_dict(sd, strict=True)
    assert not ret.missing_keys and not ret.unexpected_keys and not fresh.frozen_bn     # (the flag does not travel)
    model.train()
    assert model.frozen_bn and model.training and not model.image_encoder.batch_stats
    model.freeze_bn(False)
    assert not model.frozen_bn and model.image_encoder.batch_stats


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
    assert L._SIGS["mc_bn_eval_coeffs"] == ([L.P] * 4 + [L.F, L.I] + [L.P] * 3, L.I)     # the old entry and its signature stay


def test_new_entries_validate_their_arguments_without_a_launch():
    lib = L.load()
    a = L.BnactArgs()
    assert lib.mc_bnact_bwd_frozen(ctypes.byref(a), None) != 0 and b"bnact" in lib.mc_last_error()
    a.x = a.scale = a.shift = 16
    a.n_img, a.hw, a.c = 1, 8, 8
    assert lib.mc_bnact_bwd_frozen(ctypes.byref(a), None) != 0 and b"bnact_bwd_frozen" in lib.mc_last_error()   # no partials / dx
    assert lib.mc_bn_eval_stats(None, None, None, None, 1e-3, 8, None, None, None, None, None) != 0
    assert b"bn_eval_stats" in lib.mc_last_error()
    assert lib.mc_bn_bwd_finalize_frozen(None, 1, 8, None, None, None, None, None) != 0
    assert b"bn_bwd_finalize_frozen" in lib.mc_last_error()
    assert lib.mc_bn_frozen_rows(None, None, 8, 8, None, None, None) != 0 and b"bn_frozen_rows" in lib.mc_last_error()


def test_rows_select_scale_moves_only_the_row_count_threshold():
    """ops.set_rows_select_scale(k): the row-streaming / tile choice is made as a call with k x the rows would make it (the frozen
    micro-batched step: k micro-batches choose like the whole batch); default 1, returns the previous factor, shape support of
    the kernels is still asked with the real shape"""
    from mammo_clip_amd import ops
    half = ops.ROWS_MIN_M // 2
    assert ops._ROWS_SELECT_X == 1
    assert ops._rows_ok(ops.ROWS_MIN_M, 24, 144, None, 0) and not ops._rows_ok(half, 24, 144, None, 0)
    assert not ops.xbwd_rows_ok(half, 144, 24) and ops.xbwd_rows_ok(ops.ROWS_MIN_M, 144, 24)
    prev = ops.set_rows_select_scale(2)
    try:
        assert prev == 1 and ops._ROWS_SELECT_X == 2
        assert ops._rows_ok(half, 24, 144, None, 0) and not ops._rows_ok(half - 1, 24, 144, None, 0)
        assert ops.xbwd_rows_ok(half, 144, 24) and ops.proj_dgrad_fusable(half, 144, 24, half // 2)
        assert not ops._rows_ok(half, 24, 20, None, 0)                 # (a width the kernel does not take stays refused)
    finally:
        assert ops.set_rows_select_scale(prev) == 2
    assert ops._ROWS_SELECT_X == 1 and not ops._rows_ok(half, 24, 144, None, 0)


# ------------------------------------------------------------------------------------------------ MBConvBlock.plan, frozen
def _plans(enc, n, H, W, recording=True):
    out, geo = [], enc.stem_geo(n, H, W)
    for blk in enc._blocks:
        out.append(blk.plan(*geo, recording))
        geo = blk.out_geo(*geo)
    return out


def _one_of_each_kind(enc, plans):
    """block index of: no expand conv; 3x3 s1; 3x3 s2; 5x5 s1; 5x5 s2 (each with an expand conv, project conv on the row-streaming
    GEMM); a late block that stores its activation (keep_act)"""
    kinds = {}
    for blk, pl in zip(enc._blocks, plans):
        a = blk.args
        key = "expand1" if a.expand == 1 else ("keep_act" if pl.keep_act else f"k{a.k}s{a.s}")
        kinds.setdefault(key, a.idx)
    assert set(kinds) == {"expand1", "k3s1", "k3s2", "k5s1", "k5s2", "keep_act"}, kinds
    return kinds


@pytest.mark.parametrize("state", ["freeze+train", "eval"])
def test_plan_in_frozen_mode_never_reads_what_the_forward_did_not_produce(state):
    """B5 at the per-GPU batch of the timed workload (where the training-mode plan DOES choose the E-free and folded forms), one
    block of each kind, recompute modes 0-4, graph recorded: frozen, no plan may be E-free, E-free stride 2 or fold BatchNorm0
    -- all three read the Gram pair of a batch-statistics forward -- and batch_stats is off while `training` follows the module"""
    enc = EfficientNet.from_name("efficientnet-b5").train()
    n, H, W = 32, 1520, 912
    base = _plans(enc, n, H, W)
    kinds = _one_of_each_kind(enc, base)
    assert base[kinds["k3s1"]].efree and base[kinds["k3s2"]].fold_bn0 and all(p.batch_stats and p.training for p in base)
    enc.set_recompute(1)
    assert _plans(enc, n, H, W)[kinds["k3s2"]].efree_s2          # (the training-mode choice the frozen plan must not make)
    if state == "eval":
        enc.eval()
    else:
        enc.freeze_bn()
    for mode in (0, 1, 2, 3, 4):
        enc.set_recompute(mode)
        ps = _plans(enc, n, H, W)
        for kind, i in kinds.items():
            p, a = ps[i], enc._blocks[i].args
            what = (state, mode, kind)
            assert not p.batch_stats and p.training == (state != "eval"), what
            assert not p.efree and not p.efree_s2 and not p.fold_bn0, what
            assert p.keep_act == base[i].keep_act and p.fuse_proj_dgrad == base[i].fuse_proj_dgrad, what
            rc = enc._blocks[i].recompute
            assert p.store_e == (a.expand != 1 and rc == 0 and not p.xdw) and p.store_d == (rc < 2) and p.store_p == (rc < 4), what
            assert not (p.xdw and rc == 0), what                 # a recorded graph in mode 0 stores e: two-launch forward
        assert not any(p.efree or p.efree_s2 or p.fold_bn0 or p.batch_stats for p in ps), (state, mode)
    # and back: the training-mode plans are what they were
    enc.set_recompute(0).train().freeze_bn(False)
    assert _plans(enc, n, H, W) == base
