"""CPU-only tests (`pytest -m "not gpu"`): C-ABI surface, host-side mirror of the reference API, error behaviour,
LR schedule, and the world_size-2 collectives (gloo).  No HIP kernel is launched here."""
import ctypes
import math
import numpy as np
import os
import re
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import lib as L  # noqa: E402
from mammo_clip_amd.breastclip import util  # noqa: E402
from mammo_clip_amd.breastclip.loss import build_loss  # noqa: E402
from mammo_clip_amd.breastclip.model import build_model  # noqa: E402
from mammo_clip_amd.breastclip.model.modules import load_image_encoder, load_projection_head, load_text_encoder  # noqa: E402
from mammo_clip_amd.breastclip.scheduler import LinearWarmupCosineAnnealingLR  # noqa: E402
from oracle import arch as oarch, bert as obert, weights as ow  # noqa: E402


def _cfg(enc="tf_efficientnetv2-detect"):
    return {"name": "clip_custom", "temperature": 0.07,
            "image_encoder": {"source": "cnn", "name": enc, "pretrained": True, "model_type": "cnn"},
            "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                             "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
            "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}


# ------------------------------------------------------------------------------------------------ C ABI
def test_library_exports_every_header_symbol():
    """every `mc_*` function declared in include/mammoclip_hip.h is exported by the built .so and bound in lib.py"""
    header = open(os.path.join(ROOT, "include", "mammoclip_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|const char\*)\s+(mc_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 40
    lib = L.load()
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, missing
    unbound = [n for n in sorted(declared) if n not in L.EXPORTS]
    assert not unbound, unbound
    assert lib.mc_version() >= 100
    assert isinstance(lib.mc_last_error(), bytes)


def test_f16_build_exports_the_same_abi():
    """the f16 storage build (libmammoclip_hip_f16.so, -DMC_F16) exports every header symbol too and says which build it is;
    lib.py picks the library by MC_STORAGE and refuses a mismatch"""
    header = open(os.path.join(ROOT, "include", "mammoclip_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|const char\*)\s+(mc_[a-z0-9_]+)\s*\(", header))
    path = os.path.join(os.path.dirname(L.LIB_PATH), "libmammoclip_hip_f16.so")
    assert os.path.exists(path), "build() makes both storage variants"
    f16 = ctypes.CDLL(path)
    missing = [n for n in sorted(declared) if not hasattr(f16, n)]
    assert not missing, missing
    assert f16.mc_storage_is_f16() == 1 and L.load().mc_storage_is_f16() == 0
    assert L.STORAGE == "bf16" and L.LIB_PATH.endswith("libmammoclip_hip.so")
    out = subprocess.run([sys.executable, "-c", "import mammo_clip_amd.lib as L, mammo_clip_amd.ops as o; L.load(); print(L.STORAGE, o.BF16, L.load().mc_storage_is_f16())"],
                         cwd=ROOT, env=dict(os.environ, MC_STORAGE="f16"), capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[-3:] == ["f16", "torch.float16", "1"], (out.stdout, out.stderr[-500:])


def test_abi_argument_validation_without_gpu():
    """argument checks run before any launch: bad calls return a non-zero status and set mc_last_error()"""
    lib = L.load()
    a = L.GemmArgs()
    assert lib.mc_gemm_bf16(ctypes.byref(a), None) != 0
    assert b"gemm" in lib.mc_last_error()
    d = L.DwconvArgs()
    assert lib.mc_dwconv_fwd(ctypes.byref(d), None) != 0
    assert lib.mc_gemm_rows_supported(240, 40) == 1 and lib.mc_gemm_rows_supported(40, 240) == 1
    assert lib.mc_gemm_rows_supported(384, 64) == 1 and lib.mc_gemm_rows_supported(1056, 176) == 1   # 128-column tiles
    assert lib.mc_gemm_rows_supported(1824, 304) == 0 and lib.mc_gemm_rows_supported(24, 20) == 0
    assert lib.mc_gemm_rows_supported(176, 1056) == 0
    assert lib.mc_wgrad_rows_supported(240, 40) == 1 and lib.mc_wgrad_rows_supported(512, 3072) == 0
    with pytest.raises(L.MammoClipHipError):
        L.call("mc_sgemm", None, 0, 0, None, 0, 0, None, 0, 0, 0, 0, 1.0, 0.0, None, None, None, None)
    # entry points beside the path and the gated-weight helper
    assert lib.mc_gate_weights_bf16(None, None, 1, 8, 8, None, None) != 0 and b"gate_weights" in lib.mc_last_error()
    assert lib.mc_image_minmax_u8(None, 0, 0, 1, None, None) != 0 and b"image_minmax" in lib.mc_last_error()
    assert lib.mc_stem_im2col_u8(None, 0, 0, 0, 0, None, 0.3, 0.0, 1, 8, 8, 0, 0, 4, 4, None, None) != 0
    assert b"stem_im2col_u8" in lib.mc_last_error()


def test_struct_layouts_match_header(tmp_path):
    """ctypes mirrors must have the C struct sizes (checked against a C compile of the header)"""
    src = '#include <stdio.h>\n#include "mammoclip_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mc_gemm_args),' \
          ' sizeof(mc_dwconv_args), sizeof(mc_bnact_args), sizeof(mc_gemm_rows_args), sizeof(mc_wgrad_rows_args),' \
          ' sizeof(mc_adamw_tensor));return 0;}\n'
    exe = str(tmp_path / "mc_sizes_test")
    with open(exe + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), exe + ".c", "-o", exe], check=True)
    sizes = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(L.GemmArgs), ctypes.sizeof(L.DwconvArgs), ctypes.sizeof(L.BnactArgs),
                     ctypes.sizeof(L.GemmRowsArgs), ctypes.sizeof(L.WgradRowsArgs), ctypes.sizeof(L.AdamwTensor)]


# ------------------------------------------------------------------------------------------------ host mirror
@pytest.mark.parametrize("enc,arch_name,n_params,n_state", [
    ("tf_efficientnetv2-detect", "efficientnet-b2", 117126403, 710),
    ("tf_efficientnet_b5_ns-detect", "efficientnet-b5", 138093873, 1056)])
def test_state_dict_layout_matches_reference_inventory(enc, arch_name, n_params, n_state):
    model = build_model(_cfg(enc), {"breast_clip": {}}, types.SimpleNamespace(vocab_size=28996))
    sd = model.state_dict()
    shapes = ow.clip_shapes(oarch.build_arch(arch_name), obert.BertShape())
    assert list(sd.keys()) == list(shapes.keys())
    assert all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    assert len(sd) == n_state and sum(p.numel() for p in model.parameters()) == n_params
    # per-block geometry == oracle table (== reference modules, tests/golden/arch_tables.json)
    for blk, ob in zip(model.image_encoder._blocks, oarch.build_arch(arch_name).blocks):
        a = blk.args
        assert (a.expand, a.k, a.s, a.cin, a.cexp, a.cout, a.cse, a.pad, a.skip) == \
               (ob.expand, ob.k, ob.s, ob.cin, ob.cexp, ob.cout, ob.cse, ob.pad, ob.skip)
    assert model.image_encoder.stem_pad == oarch.build_arch(arch_name).stem_pad
    # strict round trip of synthetic reference-layout weights
    model.load_state_dict(ow.synth_state_dict(shapes, seed=3), strict=True)


def test_factories_error_behaviour_matches_reference():
    with pytest.raises(KeyError, match="Not supported model"):
        build_model({"name": "nope"}, {}, None)
    with pytest.raises(KeyError, match="Not supported image encoder"):
        load_image_encoder({"source": "cnn", "name": "resnet18"})
    with pytest.raises(KeyError, match="Not supported text encoder"):
        load_text_encoder({"source": "local", "name": "x", "pretrained": False}, 10)
    with pytest.raises(KeyError):
        load_projection_head(8, {"name": "conv", "proj_dim": 4})
    with pytest.raises(KeyError, match="Unknown loss"):
        build_loss({"triplet": {"loss_ratio": 1.0}})
    lf = build_loss({"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0),
                     "breast_clip_contrastive": dict(loss_ratio=0.0)})
    assert [l.name for l in lf.loss_list] == ["contrastive"] and lf.loss_list[0].loss_ratio == 1.0


def test_checkpoint_round_trip_reference_layout(tmp_path):
    """.tar checkpoints use the reference's dict layout and state_dict keys (trainer.py:215-237)"""
    from mammo_clip_amd.checkpoint import load_checkpoint, save_checkpoint
    model = build_model(_cfg(), {"breast_clip": {}}, types.SimpleNamespace(vocab_size=28996))
    shapes = ow.clip_shapes(oarch.build_arch("efficientnet-b2"), obert.BertShape())
    model.load_state_dict(ow.synth_state_dict(shapes, seed=5), strict=True)
    opt = torch.optim.AdamW(model.parameters(), lr=5e-5, weight_decay=1e-4)
    sch = LinearWarmupCosineAnnealingLR(opt, total_steps=10, warmup_steps=2)
    path = str(tmp_path / "model-epoch-3.tar")
    save_checkpoint(path, model, opt, sch, config={"base": {"seed": 10}}, epoch=3, train_loss=1.25, best=True)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(raw.keys()) == ["config", "epoch", "model", "optimizer", "scheduler", "train_loss"]
    assert list(raw["model"].keys()) == list(shapes.keys()) and raw["epoch"] == 3
    assert all(v.dtype == torch.float32 for k, v in raw["model"].items() if "num_batches" not in k and "position_ids" not in k)
    assert (tmp_path / "model-best.tar").exists()
    other = build_model(_cfg(), {"breast_clip": {}}, types.SimpleNamespace(vocab_size=28996))
    ck = load_checkpoint(path, other, strict=True)
    assert ck["train_loss"] == 1.25
    for (k, a), (_, b) in zip(model.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    # a DDP-wrapped save ("module." prefix) loads too
    torch.save({"model": {"module." + k: v for k, v in raw["model"].items()}}, str(tmp_path / "ddp.tar"))
    load_checkpoint(str(tmp_path / "ddp.tar"), other, strict=True)


def test_loss_scaler_state_travels_with_the_checkpoint(tmp_path):
    """engine.LossScaler (GradScaler's policy for the f16 storage build) exposes state_dict / load_state_dict and the
    checkpoint carries it under an extra key; before its first use the state is host-side, so this runs on CPU"""
    from mammo_clip_amd import engine
    from mammo_clip_amd.checkpoint import load_checkpoint, save_checkpoint
    sc = engine.LossScaler(init_scale=4096.0, growth_interval=7)
    assert sc.scale == 4096.0 and sc.skipped == 0 and sc.dynamic
    sd = sc.state_dict()
    assert sd["scale"] == 4096.0 and sd["growth_interval"] == 7 and sd["growth_tracker"] == 0
    model = torch.nn.Linear(2, 2)
    path = str(tmp_path / "m-epoch-1.tar")
    save_checkpoint(path, model, scaler=sc)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert raw["scaler"] == sd and "model" in raw
    sc2 = engine.LossScaler()
    load_checkpoint(path, torch.nn.Linear(2, 2), scaler=sc2)
    assert sc2.state_dict() == sd and sc2.scale == 4096.0


def test_collectives_requirement_is_checked_up_front():
    """one collective code path on every backend needs the tensor collectives + ReduceOp.AVG: probed when a Trainer meets a
    process group, with a clear message -- this torch has them"""
    from mammo_clip_amd.breastclip.util.dist_autograd import MIN_TORCH, require_tensor_collectives
    require_tensor_collectives()
    assert tuple(int(v) for v in torch.__version__.split("+")[0].split(".")[:2]) >= MIN_TORCH


def test_round5_host_policies_of_the_library():
    """pure host functions of the C ABI (no device needed): which shapes the round-5 fused launches take, and the split-K cost
    model of the TN weight-gradient kernel (values pinned to the sweep in scripts/tn_split_sweep.py)"""
    import ctypes as C
    from mammo_clip_amd import lib as L
    lib = L.load()
    # expand-conv backward in one pass: the expand geometries of EfficientNet-B2 / -B5, nothing wider than 64 input channels
    assert all(lib.mc_xbwd_rows_supported(n, k) for n, k in ((96, 16), (144, 24), (240, 40), (288, 48), (384, 64)))
    assert not any(lib.mc_xbwd_rows_supported(n, k) for n, k in ((768, 128), (528, 88), (100, 20), (384, 96)))
    # fused depthwise backward: 3x3, stride 1, with the BatchNorm epilogue operands; preferred from 192 channels on the wide
    # and the narrow maps of the networks
    def dw(c, k, s, h, w, n=32, epi=True):
        a = L.DwconvArgs()
        a.n, a.h, a.w, a.c, a.k, a.stride, a.pad_l, a.pad_t, a.oh, a.ow = n, h, w, c, k, s, (k - 1) // 2, (k - 1) // 2, h, w
        a.epi_x = 16 if epi else None
        return a
    assert lib.mc_dwconv_bwd_fused_supported(C.byref(dw(240, 3, 1, 380, 228))) and lib.mc_dwconv_bwd_fused_preferred(C.byref(dw(240, 3, 1, 380, 228)))
    assert lib.mc_dwconv_bwd_fused_preferred(C.byref(dw(768, 3, 1, 95, 57))) and lib.mc_dwconv_bwd_fused_preferred(C.byref(dw(3072, 3, 1, 48, 29)))
    assert lib.mc_dwconv_bwd_fused_supported(C.byref(dw(24, 3, 1, 760, 456))) and not lib.mc_dwconv_bwd_fused_preferred(C.byref(dw(24, 3, 1, 760, 456)))
    assert not lib.mc_dwconv_bwd_fused_supported(C.byref(dw(384, 5, 1, 190, 114)))          # 5x5: does not fit a wave's registers
    assert not lib.mc_dwconv_bwd_fused_supported(C.byref(dw(240, 3, 1, 380, 228, epi=False)))
    assert not lib.mc_dwconv_bwd_fused_supported(C.byref(dw(144, 3, 2, 760, 456)))
    # TN split-K: round count x K tiles + workspace traffic
    assert lib.mc_gemm256_tn_splits(512, 3072, 44544, 0) == 8 and lib.mc_gemm256_tn_splits(3072, 512, 44544, 0) == 8
    assert lib.mc_gemm256_tn_splits(176, 1056, 173280, 0) == 48 and lib.mc_gemm256_tn_splits(304, 1824, 44544, 0) == 16
    assert lib.mc_gemm256_tn_splits(3072, 768, 16384, 0) == 7 and lib.mc_gemm256_tn_splits(768, 768, 16384, 0) == 24


def _span(*ranges):
    return [i for lo, hi in ranges for i in range(lo, hi + 1)]


_PLAN_TABLE = [
    ("efficientnet-b5", 32, 1520, 912, dict(xdw_ok=_span((3, 13)), efree=_span((4, 7)), fused_dw=_span((4, 7), (14, 19), (36, 38)),
                                            fold_bn0=_span((3, 27), (37, 38)), no_keep_act=_span((0, 12)), fuse_proj_dgrad=_span((3, 7)))),
    ("efficientnet-b2", 64, 912, 912, dict(xdw_ok=_span((2, 8)), efree=_span((3, 4)), fused_dw=_span((3, 4), (9, 11), (21, 22)),
                                           fold_bn0=_span((2, 8), (13, 16)), no_keep_act=_span((0, 7)), fuse_proj_dgrad=_span((3, 4)))),
]


def test_mbconv_plan_of_every_block():
    """MBConvBlock.plan (the one place where the forward / backward paths of a block call are chosen) needs no device: the
    library's shape predicates are host functions.  Pinned per block (``blk.args.idx``) at the per-GPU batch of the timed
    workloads, default switches and thresholds, bf16: a changed threshold or library predicate shows up HERE.  The lists are
    what the separate forward / backward conditions of the code before ``plan`` gave at these shapes ("B5 blocks
    4-7", "B2 blocks 3-4")."""
    for name, n, H, W, want in _PLAN_TABLE:
        _check_plans(name, n, H, W, want)


def _check_plans(name, n, H, W, want):
    from mammo_clip_amd.breastclip.model.modules.efficientnet_custom import EfficientNet
    enc = EfficientNet.from_name(name).train()

    def plans(recording):
        out, geo = [], enc.stem_geo(n, H, W)
        for blk in enc._blocks:
            out.append(blk.plan(*geo, recording))
            assert (out[-1].n, out[-1].oh, out[-1].ow) == blk.out_geo(*geo)
            geo = blk.out_geo(*geo)
        return out

    def idx(ps, field, value=True):
        return [i for i, p in enumerate(ps) if getattr(p, field) == value]

    assert [blk.args.idx for blk in enc._blocks] == list(range(len(enc._blocks)))
    has_expand = [blk.args.idx for blk in enc._blocks if blk.args.expand != 1]
    # training, recompute 0, graph recorded: only the E-free blocks run the fused forward, every other block stores e
    ps = plans(True)
    assert idx(ps, "efree") == want["efree"] and idx(ps, "xdw") == want["efree"]
    assert idx(ps, "fused_dw") == want["fused_dw"] and idx(ps, "fold_bn0") == want["fold_bn0"]
    assert idx(ps, "keep_act", False) == want["no_keep_act"] and idx(ps, "fuse_proj_dgrad") == want["fuse_proj_dgrad"]
    assert idx(ps, "store_e") == [i for i in has_expand if i not in want["efree"]]
    assert all(p.store_d and p.store_p and not p.fp8_expand and not p.fp8_project and p.training for p in ps)
    assert all(p.fused_dw and p.fold_bn0 for p in ps if p.efree) and not any(p.xbwd and p.fold_bn0 for p in ps)
    # no graph: the whole eligible column runs the fused forward
    ps = plans(False)
    assert idx(ps, "xdw") == want["xdw_ok"] and idx(ps, "efree") == want["efree"]
    # recompute modes (EfficientNet.set_recompute): 1 drops e, 2 also d, 4 also p; 3 = 2 on the stride-1 3x3 blocks with an
    # expand conv, 1 elsewhere
    for mode in (1, 2, 3, 4):
        enc.set_recompute(mode)
        ps = plans(True)
        assert idx(ps, "xdw") == want["xdw_ok"] and idx(ps, "efree") == want["efree"] and idx(ps, "store_e") == []
        mode2 = [b.args.idx for b in enc._blocks if b.args.k == 3 and b.args.s == 1 and b.args.expand != 1]
        assert idx(ps, "store_d", False) == {1: [], 2: list(range(len(ps))), 3: mode2, 4: list(range(len(ps)))}[mode]
        assert idx(ps, "store_p", False) == (list(range(len(ps))) if mode == 4 else [])
    enc.set_recompute(0)
    # fp8 operands: neither fused forward nor E-free
    enc.set_fp8(True)
    ps = plans(True)
    assert idx(ps, "xdw") == [] and idx(ps, "efree") == []
    enc.set_fp8(False)
    # eval: no E-free block; the eligible column still runs the fused forward (nothing is stored)
    enc.eval()
    with torch.no_grad():
        ps = plans(False)
    assert idx(ps, "efree") == [] and idx(ps, "xdw") == want["xdw_ok"] and not any(p.training for p in ps)


def test_no_cpu_fallback():
    """the product path refuses CPU tensors instead of silently computing somewhere else"""
    model = build_model(_cfg(), {"breast_clip": {}}, types.SimpleNamespace(vocab_size=28996))
    with pytest.raises(RuntimeError, match="HIP device"):
        model.image_encoder(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="HIP device"):
        model.text_encoder({"input_ids": torch.zeros(1, 8, dtype=torch.long), "attention_mask": torch.ones(1, 8, dtype=torch.long)})
    with pytest.raises(RuntimeError, match="HIP device"):
        model.image_projection(torch.zeros(2, 1408))
    from mammo_clip_amd.breastclip.optimizer import AdamW
    w = torch.nn.Parameter(torch.zeros(4))
    w.grad = torch.ones(4)
    with pytest.raises(L.MammoClipHipError, match="only path"):
        AdamW([w], lr=1e-3).step()
    lib = L.load()
    assert lib.mc_adamw_step(None, 3, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) != 0     # null list
    assert lib.mc_adamw_step(None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None) != 0     # step must be >= 1


def test_global_env_and_scheduler():
    util.GlobalEnv.reset()
    env = util.GlobalEnv.get()
    assert (env.world_size, env.world_rank, env.master) == (1, 0, True)
    assert env.summary_writer.train is None and env.summary_writer.global_step == 0
    with pytest.raises(Exception, match="singleton"):
        util.GlobalEnv()
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sch = LinearWarmupCosineAnnealingLR(opt, total_steps=10, warmup_steps=2)
    lrs = []
    for _ in range(10):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    ref = [0.0, 0.5] + [math.cos((s - 2) / 8 * math.pi / 2) ** 2 for s in range(2, 10)]   # warmup_cosine.py:41-50
    assert all(abs(a - b) < 1e-9 for a, b in zip(lrs, ref))


def test_build_scheduler_matches_reference_config_shapes():
    """[ref: scheduler/__init__.py:8-16 + trainer_ddp.py:146-153]: resolved step configs, epoch configs with an int
    warm-up (epochs) and with a float warm-up (fraction of the total steps, e.g. cosine_epoch30_warmup3.yaml's 0.1),
    and the 'constant' schedule = torch's ConstantLR with the config passed through."""
    from mammo_clip_amd.breastclip.scheduler import build_scheduler

    def opt():
        return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    s1 = build_scheduler(opt(), {"name": "cosine", "config": {"total_steps": 100, "warmup_steps": 10}})
    assert (s1.tsteps, s1.wsteps) == (100, 10)
    s2 = build_scheduler(opt(), {"name": "cosine", "config": {"total_epochs": 30, "warmup_epochs": 3}}, steps_per_epoch=500)
    assert (s2.tsteps, s2.wsteps) == (15000, 1500)
    s3 = build_scheduler(opt(), {"name": "cosine", "config": {"total_epochs": 30, "warmup_epochs": 0.1}}, steps_per_epoch=500)
    assert (s3.tsteps, s3.wsteps) == (15000, 1500)            # 0.1 of the total, NOT 0.1 * steps_per_epoch
    s4 = build_scheduler(opt(), {"name": "cosine", "config": {"total_steps": 7, "warmup_steps": 2}}, total_steps=50)
    assert (s4.tsteps, s4.wsteps) == (50, 2)
    o = opt()
    s5 = build_scheduler(o, {"name": "constant", "config": {"factor": 0.5, "total_iters": 2}})
    assert isinstance(s5, torch.optim.lr_scheduler.ConstantLR)
    lrs = []
    for _ in range(4):
        lrs.append(o.param_groups[0]["lr"]); o.step(); s5.step()
    assert lrs == [0.5, 0.5, 1.0, 1.0]
    assert isinstance(build_scheduler(opt(), {"name": "constant", "config": {}}), torch.optim.lr_scheduler.ConstantLR)
    with pytest.raises(NotImplementedError):
        build_scheduler(opt(), {"name": "step", "config": {}})


def test_custom_ops_registered_with_torch_library():
    """the kernels are dispatcher-visible operators (``torch.ops.mammoclip.*``) with schemas and fake (meta)
    implementations; the real implementation exists for device type cuda only (CPU tensors raise: no fallback)."""
    import mammo_clip_amd.custom_ops as co
    for name in co.OPS:
        assert hasattr(torch.ops.mammoclip, name), name
    x = torch.empty(10, 16, dtype=torch.bfloat16, device="meta")
    w = torch.empty(24, 16, dtype=torch.bfloat16, device="meta")
    assert torch.ops.mammoclip.linear(x, w).shape == (10, 24)
    assert torch.ops.mammoclip.linear_wgrad(torch.empty(10, 24, dtype=torch.bfloat16, device="meta"), x).dtype == torch.float32
    d = torch.ops.mammoclip.dwconv(torch.empty(2 * 6 * 6, 8, dtype=torch.bfloat16, device="meta"),
                                   torch.empty(9, 8, device="meta"), 2, 6, 6, 3, 2, 0, 0, 3, 3)
    assert d.shape == (2 * 3 * 3, 8)
    assert "Tensor? bias=None" in str(torch.ops.mammoclip.linear.default._schema)
    # the operators the MODEL's 1x1-convolution / depthwise launches go through (ops.linear_fwd & co. are wrappers over them)
    y, part = torch.ops.mammoclip.conv1x1(x, w, None, None, None, None, None, 0, True, False)
    assert y.shape == (10, 24) and part.shape[1:] == (2, 24) and part.dtype == torch.float32
    assert torch.ops.mammoclip.conv1x1_wgrad(y, x, None, None, None, 0, False).shape == (24, x.shape[1])
    dd, dpart = torch.ops.mammoclip.dwconv_bn(torch.empty(2 * 6 * 6, 8, dtype=torch.bfloat16, device="meta"),
                                              torch.empty(9, 8, device="meta"), 2, 6, 6, 3, 2, 0, 0, 3, 3, None, None, False)
    assert dd.shape == (2 * 3 * 3, 8) and dpart.numel() == 0
    import inspect
    from mammo_clip_amd import ops
    for fn in (ops.linear_fwd, ops.linear_dgrad, ops.linear_wgrad, ops.dwconv_fwd, ops.dwconv_bwd_data, ops.dwconv_bwd_weight):
        assert "_OP_" in inspect.getsource(fn), fn.__name__          # = torch.ops.mammoclip.<name>.default, bound at import
    assert ops._OP_CONV1X1 is torch.ops.mammoclip.conv1x1.default and ops._OP_DWCONV_BN is torch.ops.mammoclip.dwconv_bn.default
    with pytest.raises(NotImplementedError):
        torch.ops.mammoclip.linear(torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16))


class _ToyModel(torch.nn.Module):
    def forward(self, batch, device=None):
        assert not self.training and not torch.is_grad_enabled()
        return {"x": batch["x"]}


class _ToyLoss:
    loss_list = [types.SimpleNamespace(name="contrastive", loss_ratio=1.0)]

    def __call__(self, x, is_train):
        assert is_train is False
        return {"contrastive": x * 2.0, "total": x}


def test_validate_matches_reference_loop_semantics():
    """row N3 [ref: trainer_ddp.py:346-409]: eval mode + no_grad, is_train=False, per-key accumulation, the
    ``idx == 10: break`` quirk (11 batches evaluated) with division by the FULL loader length"""
    from mammo_clip_amd.engine import validate
    loader = [{"x": torch.tensor(float(i))} for i in range(13)]
    m = _ToyModel().train()
    res = validate(m, _ToyLoss(), {"vindr": loader, "upmc": loader[:2]})
    assert not m.training
    assert abs(res["vindr"]["total"] - sum(range(11)) / 13) < 1e-6
    assert abs(res["vindr"]["contrastive"] - 2 * sum(range(11)) / 13) < 1e-6
    assert abs(res["upmc"]["total"] - 0.5) < 1e-6
    from mammo_clip_amd.breastclip.evaluator import Evaluator
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((5, 16)), rng.standard_normal((3, 16))
    from scipy.special import softmax
    from sklearn import metrics
    np.testing.assert_allclose(Evaluator.zeroshot_scores(a, b), softmax(metrics.pairwise.cosine_similarity(a, b), axis=1),
                               rtol=1e-12, atol=1e-12)                  # evaluator.py:171


# ------------------------------------------------------------------------------------------------ world_size = 2 (gloo)
def _w2_worker(rank, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    # ONE collective code path for every backend: the list forms must never be reached, and the tensor forms /
    # all_reduce(AVG) that tests/test_dist_gpu.py counts over RCCL are the ones counted here over gloo
    calls = {"all_gather_into_tensor": 0, "reduce_scatter_tensor": 0, "all_reduce_avg": 0}
    _ag, _rs, _ar = dist.all_gather_into_tensor, dist.reduce_scatter_tensor, dist.all_reduce

    def ag(*a_, **k_):
        calls["all_gather_into_tensor"] += 1
        return _ag(*a_, **k_)

    def rs(*a_, **k_):
        calls["reduce_scatter_tensor"] += 1
        return _rs(*a_, **k_)

    def ar(t_, op=dist.ReduceOp.SUM, **k_):
        calls["all_reduce_avg"] += int(op == dist.ReduceOp.AVG)
        return _ar(t_, op=op, **k_)
    dist.all_gather_into_tensor, dist.reduce_scatter_tensor, dist.all_reduce = ag, rs, ar
    dist.all_gather = dist.reduce_scatter = None
    sys.path.insert(0, ROOT)
    import mammo_clip_amd  # noqa: F401
    from mammo_clip_amd.breastclip import util as U
    from mammo_clip_amd.breastclip.util.dist_autograd import DistAutogradAllGatherFunction, all_gather_fused
    from mammo_clip_amd.engine import GradBuckets
    U.GlobalEnv.reset()
    env = U.GlobalEnv.get()
    assert (env.world_size, env.world_rank) == (2, rank)
    g = torch.Generator().manual_seed(7)
    full = [torch.randn(6, 5, generator=g) for _ in range(3)]
    local = [f[rank * 3:(rank + 1) * 3].clone().requires_grad_(True) for f in full]
    gathered = all_gather_fused(local)
    ok = all(torch.equal(ga, f) for ga, f in zip(gathered, full))
    w = [torch.randn(6, 5, generator=g) for _ in range(3)]
    loss = sum((ga * wi).sum() * (rank + 1) for ga, wi in zip(gathered, w))       # rank-dependent loss
    loss.backward()
    # reduce_scatter(SUM): d/d local = sum over ranks q of (q+1) * w[slice of this rank]
    ok = ok and all(torch.allclose(l.grad, 3.0 * wi[rank * 3:(rank + 1) * 3]) for l, wi in zip(local, w))
    # reference-style per-tensor function gives the same gather
    F = DistAutogradAllGatherFunction(partial=False)
    t = full[0][rank * 3:(rank + 1) * 3].clone().requires_grad_(True)
    cat = torch.cat(F.apply(t), 0)
    ok = ok and torch.equal(cat, full[0])
    (cat * w[0]).sum().backward()
    ok = ok and torch.allclose(t.grad, 2.0 * w[0][rank * 3:(rank + 1) * 3])
    # bucketed gradient averaging, with one parameter that never receives a gradient (like the BERT pooler)
    params = [torch.nn.Parameter(torch.full((4,), float(i))) for i in range(5)]
    gb = GradBuckets(params, bucket_bytes=32)
    gb.begin()
    for i, p in enumerate(params[:4]):
        (p.sum() * (rank + 1) * (i + 1)).backward()
    gb.finish()
    ok = ok and all(torch.allclose(p.grad, torch.full((4,), 1.5 * (i + 1))) for i, p in enumerate(params[:4]))
    ok = ok and params[4].grad is None
    # micro-batched steps: hooks off, several backward calls, one collection + reduction at the end
    params2 = [torch.nn.Parameter(torch.full((3,), float(i))) for i in range(4)]
    gb2 = GradBuckets(params2, bucket_bytes=16)
    gb2.begin()
    gb2.enabled = False
    for rep in range(2):
        for i, p in enumerate(params2[:3]):
            (p.sum() * (rank + 1) * (i + 1)).backward()
    gb2.enabled = True
    gb2.reduce_all()
    ok = ok and all(torch.allclose(p.grad, torch.full((3,), 2 * 1.5 * (i + 1))) for i, p in enumerate(params2[:3]))
    ok = ok and params2[3].grad is None
    # ... and the overlapped form the micro-batched step uses: hooks off for the first pass, ON for the last one (each
    # bucket is reduced from the hook that completes it), a parameter whose gradient only exists from the first pass
    # (like logit_scale, which only the loss backward touches) is picked up by finish()
    params3 = [torch.nn.Parameter(torch.full((3,), float(i))) for i in range(5)]
    gb3 = GradBuckets(params3, bucket_bytes=16)
    gb3.begin()
    gb3.enabled = False
    for i, p in enumerate(params3[:4]):
        (p.sum() * (rank + 1) * (i + 1)).backward()
    gb3.enabled = True
    for i, p in enumerate(params3[:3]):
        (p.sum() * (rank + 1) * (i + 1)).backward()
    gb3.finish()
    ok = ok and all(torch.allclose(p.grad, torch.full((3,), 2 * 1.5 * (i + 1))) for i, p in enumerate(params3[:3]))
    ok = ok and torch.allclose(params3[3].grad, torch.full((3,), 1.5 * 4)) and params3[4].grad is None
    # a backward outside begin()/finish() (buckets not armed) is plain autograd
    (params3[0].sum() * 2.0).backward()
    # Trainer construction puts rank 0's parameters and buffers on every rank (DDP's construction-time broadcast)
    from mammo_clip_amd.engine import Trainer
    torch.manual_seed(100 + rank)
    toy = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    toy[1].running_mean.fill_(float(rank))
    Trainer(toy, None, None)
    torch.manual_seed(100)
    ref_toy = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    ok = ok and all(torch.equal(a, b) for a, b in zip(toy.parameters(), ref_toy.parameters()))
    ok = ok and float(toy[1].running_mean[0]) == 0.0
    # buffers of rank 0 everywhere (DDP broadcast_buffers semantics), mixed dtypes
    from mammo_clip_amd.engine import sync_buffers
    bn = torch.nn.BatchNorm2d(3)
    bn.running_mean.fill_(float(rank + 1)); bn.running_var.fill_(float(10 * (rank + 1))); bn.num_batches_tracked.fill_(7 * (rank + 1))
    sync_buffers(bn)
    ok = ok and float(bn.running_mean[0]) == 1.0 and float(bn.running_var[2]) == 10.0 and int(bn.num_batches_tracked) == 7
    # validation pass: per-batch mean over ranks [ref: trainer_ddp.py:384-387]
    from mammo_clip_amd.engine import validate
    res = validate(_ToyModel(), _ToyLoss(), {"d": [{"x": torch.tensor(float(rank + 1 + i))} for i in range(3)]})
    ok = ok and abs(res["d"]["total"] - (1.5 + 2.5 + 3.5) / 3) < 1e-6
    ok = ok and calls["all_gather_into_tensor"] >= 2 and calls["reduce_scatter_tensor"] >= 2 and calls["all_reduce_avg"] >= 1
    ret[rank] = bool(ok)
    dist.destroy_process_group()


def test_world2_gather_reduce_scatter_and_grad_buckets():
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_w2_worker, args=(29731, ret), nprocs=2, join=True)
    assert ret[0] and ret[1]


def test_grad_sink_sums_like_autograd():
    """ops.GradSink: contributions of one backward call are summed among themselves, then added to the accumulator of
    earlier calls (autograd's order); parameters without a contribution keep grad None; finish() adds to an existing
    ``.grad`` (parameters that also receive plain autograd gradients)."""
    import torch
    from mammo_clip_amd import ops
    p1, p2, p3 = (torch.nn.Parameter(torch.zeros(s)) for s in ((3,), (2, 2), (4,)))
    sk = ops.GradSink()
    sk.deliver([p1, p2], [torch.full((3,), 1.0), torch.full((2, 2), 0.5)])
    sk.deliver([p1], [torch.full((3,), 2.0)])
    sk.flush()
    sk.deliver([p1, p2], [torch.full((3,), 4.0), None])
    sk.deliver([p1], [torch.full((3,), 8.0)])
    sk.deliver([p1], [torch.full((3,), 16.0)])
    p2.grad = torch.ones(2, 2)
    sk.finish()
    assert torch.equal(p1.grad, torch.full((3,), 31.0)) and torch.equal(p2.grad, torch.full((2, 2), 1.5)) and p3.grad is None
    assert not sk.acc and not sk.pending
    # no sink installed: the backward functions return their gradients to autograd unchanged
    assert ops.GRAD_SINK is None and ops.deliver_param_grads([p1], [p1.grad]) == (p1.grad,)


def test_trainer_step_failure_leaves_no_gradient_sink_behind():
    """a step that raises (OOM, a data error in a re-forward) must not leave the module-level gradient sink
    installed or carry partial gradients into the next step; a backward outside the Trainer sees plain autograd."""
    import torch
    from mammo_clip_amd import engine, ops

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(3))
            self.fail = False

        def forward(self, batch, device=None):
            if self.fail:
                raise RuntimeError("data error")

            class F_(torch.autograd.Function):            # hands its parameter gradient to the sink like the HIP functions
                @staticmethod
                def forward(ctx, x, w):
                    ctx.save_for_backward(x)
                    return x * w

                @staticmethod
                def backward(ctx, g):
                    (x,) = ctx.saved_tensors
                    (gw,) = ops.deliver_param_grads([self.w], [(g * x).clone()])
                    return None, gw
            return {"y": F_.apply(batch["x"], self.w)}

    def loss(y, is_train):
        return {"total": y.sum()}
    m = Toy()
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    tr = engine.Trainer(m, loss, opt, None, None)
    tr.step({"x": torch.tensor([1.0, 2.0, 3.0])})
    assert ops.GRAD_SINK is None and tr._sink is None and torch.equal(m.w.grad, torch.tensor([1.0, 2.0, 3.0]))
    m.fail = True
    with pytest.raises(RuntimeError, match="data error"):
        tr.step({"x": torch.ones(3)})
    assert ops.GRAD_SINK is None and tr._sink is None
    # a failure INSIDE a backward call (sink installed at that moment)
    m.fail = False

    def bad_loss(y, is_train):
        class G_(torch.autograd.Function):
            @staticmethod
            def forward(ctx, v):
                return v.sum()

            @staticmethod
            def backward(ctx, g):
                raise RuntimeError("backward error")
        return {"total": G_.apply(y)}
    tr.loss_func = bad_loss
    with pytest.raises(RuntimeError, match="backward error"):
        tr.step({"x": torch.ones(3)})
    assert ops.GRAD_SINK is None and tr._sink is None
    # the next good step starts clean, and a backward outside the Trainer delivers through autograd
    tr.loss_func = loss
    tr.step({"x": torch.tensor([2.0, 2.0, 2.0])})
    assert torch.equal(m.w.grad, torch.tensor([2.0, 2.0, 2.0]))
    m.zero_grad(set_to_none=True)
    m({"x": torch.ones(3)})["y"].sum().backward()
    assert torch.equal(m.w.grad, torch.ones(3))


def test_side_view_running_statistics_are_applied_in_the_reference_order():
    """Launch chains (model/clip.py MC_STREAMS): the second image view runs beside the first one, so its BatchNorm finalize
    launches must not touch the running statistics -- they update zero-filled scratch slices (-> m * s) and _BNDefer.apply
    folds them in after the join: r <- (1 - m) r + (m s), behind view 1's update, i.e. the reference's two sequential
    encode_image calls [ref: model/clip.py:83,108].  Host logic only: offsets of the flat scratch buffer, which layers were
    touched, the arithmetic of apply (the kernels' side is tests/test_model_gpu.py::test_encoder_chains_on_side_streams_same_step),
    and the cache keys warm_weight_images must hit are the ones the autograd functions ask for."""
    from mammo_clip_amd.breastclip.model.modules import efficientnet_custom as ec
    enc = load_image_encoder({"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": False, "model_type": "cnn"})
    bns = enc._bn_layers
    assert len(bns) == sum(1 for m in enc.modules() if isinstance(m, ec._BN)) and len(bns) > 60
    g = torch.Generator().manual_seed(3)
    for bn in bns:
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g))
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
    m = ec.BN_MOMENTUM
    d = ec._BNDefer(enc)
    assert d.flat.numel() == 2 * sum(bn.num_features for bn in bns) and float(d.flat.abs().max()) == 0.0
    want, seen = {}, set()
    for bn in bns[::3]:                                        # a forward that touches every third layer
        rm, rv = d.scratch(bn)
        assert rm.shape == rv.shape == (bn.num_features,)
        assert (rm.data_ptr(), rv.data_ptr()) not in seen      # disjoint slices
        seen.add((rm.data_ptr(), rv.data_ptr()))
        s_mean, s_var = torch.randn(bn.num_features, generator=g), torch.rand(bn.num_features, generator=g)
        rm.copy_(m * s_mean)                                   # what bn_finalize_k leaves: (1 - m) * 0 + m * s
        rv.copy_(m * s_var)
        want[id(bn)] = ((1.0 - m) * bn.running_mean + m * s_mean, (1.0 - m) * bn.running_var + m * s_var)
    untouched = {id(bn): (bn.running_mean.clone(), bn.running_var.clone()) for bn in bns if id(bn) not in want}
    d.apply()
    for bn in bns:
        if id(bn) in want:
            torch.testing.assert_close(bn.running_mean, want[id(bn)][0], rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(bn.running_var, want[id(bn)][1], rtol=1e-6, atol=1e-7)
        else:
            assert torch.equal(bn.running_mean, untouched[id(bn)][0]) and torch.equal(bn.running_var, untouched[id(bn)][1])
    assert d.used == []                                        # applied once
    # side_call_begin / side_call_end bracket: counters are held back, the deferral object is installed only in training mode
    enc.eval()
    enc.side_call_begin()
    assert enc._side_defer is None and enc._side_counters == []
    assert enc._new_call().counters is enc._side_counters      # (held: a call inside the bracket collects into the bracket's list)
    enc.side_call_end()
    assert enc._side_counters is None
    enc.train()
    enc.side_call_begin()
    assert isinstance(enc._side_defer, ec._BNDefer) and enc._new_call().defer is enc._side_defer
    enc.side_call_end()
    assert enc._side_defer is None and enc._side_counters is None


def test_encoder_call_context_host_logic(monkeypatch):
    """``_Call``, the per-forward context of the image encoder: where a BatchNorm site's finalize launch sends its running-statistic
    update, which batch counters the call collects, what a statistics tape records and replays -- and that all of it lives in the
    context, so a forward that dies half-way leaves nothing on the encoder or its layers.  Host logic only: ops.bn_finalize /
    ops.bn_eval_coeffs are recording stubs."""
    from mammo_clip_amd.breastclip.model.modules import efficientnet_custom as ec
    enc = load_image_encoder({"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": False, "model_type": "cnn"})
    bns = enc._bn_layers[:4]
    fin, coef, fail_at = [], [], [None]

    def bn_finalize(partials, count, w, b, rm, rv, momentum, eps, update):
        if fail_at[0] == len(fin):
            raise RuntimeError("finalize failed")
        fin.append((rm, rv, update))
        return object()
    monkeypatch.setattr(ec.ops, "bn_finalize", bn_finalize)
    monkeypatch.setattr(ec.ops, "bn_eval_coeffs", lambda w, b, rm, rv, eps: coef.append((rm, rv)) or "eval")
    state = lambda: (dict(enc.__dict__), [sorted(bn.__dict__) for bn in enc._bn_layers])      # noqa: E731
    clean = state()
    # default context: the layer's own buffers, update on, the layer's counter collected
    call = enc._new_call()
    assert (call.tape, call.update_running, call.defer, call.counters, call.head) == (None, True, None, [], None)
    for bn in bns:
        ec._bn_stats(call, None, 8, bn, True)
    assert all(rm is bn.running_mean and rv is bn.running_var and upd is True for (rm, rv, upd), bn in zip(fin, bns))
    assert len(call.counters) == 4 and all(c is bn.num_batches_tracked for c, bn in zip(call.counters, bns))
    # a side chain: the scratch slices of its _BNDefer, the layer marked used
    d = ec._BNDefer(enc)
    call, n0 = enc._new_call(d), len(fin)
    for bn in bns[:2]:
        ec._bn_stats(call, None, 8, bn, True)
    for (rm, rv, upd), bn in zip(fin[n0:], bns):
        o = d.offs[id(bn)]
        assert upd is True and rm.data_ptr() == d.flat[o:].data_ptr() and rv.data_ptr() == d.flat[d.total + o:].data_ptr()
        assert rm.shape == rv.shape == (bn.num_features,)
    assert d.used == bns[:2] and len(call.counters) == 2
    # updates off (the engine's re-forwards): update=False reaches the launch, no counter, the deferral object is ignored
    d = ec._BNDefer(enc)
    enc.update_running = False
    call, n0 = enc._new_call(d), len(fin)
    enc.update_running = True
    ec._bn_stats(call, None, 8, bns[0], True)
    assert fin[n0][0] is bns[0].running_mean and fin[n0][1] is bns[0].running_var and fin[n0][2] is False
    assert call.counters == [] and d.used == []
    # record, then replay: the identical objects in order, no launch; inactive sites run fn and stay off the tape
    tape = ec.StatTape()
    enc.set_stat_tape(tape)
    call = enc._new_call()
    rec = [ec._bn_stats(call, None, 8, bns[0], True), call.taped(True, lambda: "gram"), call.taped(True, lambda: "pooled"),
           ec._bn_stats(call, None, 8, bns[1], True)]
    assert call.taped(False, lambda: "off") == "off" and not call.replaying
    assert tape.items == rec and len(call.counters) == 2
    enc.set_stat_tape(tape.replay())
    call, n0 = enc._new_call(), len(fin)
    enc.set_stat_tape(None)

    def never():
        raise AssertionError("a replay computes nothing")
    got = [ec._bn_stats(call, None, 8, bns[0], True), call.taped(True, never), call.taped(True, never),
           ec._bn_stats(call, None, 8, bns[1], True)]
    assert call.replaying and call.taped(False, lambda: "off") == "off"
    assert all(g is r for g, r in zip(got, rec)) and tape.pos == len(tape.items) == 4
    assert len(fin) == n0 and call.counters == []
    # ... and a replay needs no statistics partials from the producers, a rebuild in the backward (no call) neither
    prod = lambda *a, stats=False: ("y", "partials") if stats else "y"      # noqa: E731
    assert ec._conv_stats(call, prod, True) == ("y", None) and ec._conv_stats(call, prod, False) == ("y", "partials")
    assert ec._conv_stats(None, prod, True, stats=False) == ("y", None)
    assert ec._conv_stats(enc._new_call(), prod, True) == ("y", "partials")
    # running statistics (eval / frozen): bn_eval_coeffs on the buffers; tape and counters are left alone
    tape = ec.StatTape()
    call, n0 = ec._Call(tape=tape, counters=[]), len(fin)
    assert ec._bn_stats(call, None, 8, bns[2], False) == "eval"
    assert coef[-1][0] is bns[2].running_mean and coef[-1][1] is bns[2].running_var
    assert len(fin) == n0 and tape.items == [] and tape.pos == 0 and call.counters == []
    # a forward that dies half-way leaves nothing behind: the next context starts clean
    tape, d = ec.StatTape(), ec._BNDefer(enc)
    enc.set_stat_tape(tape)
    call = enc._new_call(d)
    enc.set_stat_tape(None)
    fail_at[0] = len(fin) + 2
    with pytest.raises(RuntimeError, match="finalize failed"):
        for bn in bns:
            ec._bn_stats(call, None, 8, bn, True)
    assert len(call.counters) == 2 and len(tape.items) == 2 and len(d.used) == 3
    after = state()
    assert after[1] == clean[1] and after[0].keys() == clean[0].keys()
    assert all(after[0][k] is clean[0][k] for k in clean[0])
    assert not any(hasattr(enc, a) for a in ("_head_cache", "_last_seed", "_pending_counters", "_hold_counters"))
    assert not any(hasattr(bn, a) for bn in enc._bn_layers for a in ("track_update", "defer_count"))
    call = enc._new_call()
    assert (call.tape, call.update_running, call.defer, call.counters, call.head) == (None, True, None, [], None)


# ------------------------------------------------------------------------------------------------ world_size = 2: the N = 8 step policy
class _ToyClip(torch.nn.Module):
    """Stand-in with the attributes engine._step_micro touches (seed counters of both encoders, the MBConv recompute switch,
    logit_scale): per-sample linear encoders, so W ranks x k micro-batches must reproduce the single-process step exactly."""

    class _Blk:
        recompute = 0

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.wi = torch.nn.Parameter(torch.randn(6, 5, generator=g) * 0.5)
        self.wt = torch.nn.Parameter(torch.randn(4, 5, generator=g) * 0.5)
        self.logit_scale = torch.nn.Parameter(torch.tensor(1.3))
        self.unused = torch.nn.Parameter(torch.zeros(2))               # like the BERT pooler: never receives a gradient
        self.image_encoder = types.SimpleNamespace(rng=types.SimpleNamespace(calls=0), _blocks=[self._Blk(), self._Blk()],
                                                   set_recompute=self._set_recompute)
        self.text_encoder = types.SimpleNamespace(_calls=0)
        self.modes_seen = []

    def _set_recompute(self, mode):
        for b in self.image_encoder._blocks:
            b.recompute = mode

    def forward(self, batch, device=None):
        self.image_encoder.rng.calls += 2
        self.text_encoder._calls += 1
        self.modes_seen.append((self.image_encoder._blocks[0].recompute, torch.is_grad_enabled()))
        n = torch.nn.functional.normalize
        return {"image_embeddings": n(batch["images"] @ self.wi), "text_embeddings": n(batch["text"] @ self.wt),
                "text_embeddings2": n(batch["text2"] @ self.wt), "image_view_embeddings": n(batch["image_views"] @ self.wi),
                "labels": torch.arange(batch["images"].shape[0]), "logit_scale": self.logit_scale.exp()}


def _toy_loss(image_embeddings, text_embeddings, text_embeddings2, image_view_embeddings, labels, logit_scale, is_train):
    """symmetric InfoNCE over the embeddings of ALL ranks (fused all-gather, reduce-scatter backward) with this rank's label
    offset -- the structure of loss/breast_clip.py on plain torch ops (the product loss launches HIP kernels)"""
    from mammo_clip_amd.breastclip import util as U
    from mammo_clip_amd.breastclip.util.dist_autograd import all_gather_fused
    env = U.GlobalEnv.get()
    loc = [image_embeddings, text_embeddings, text_embeddings2, image_view_embeddings]
    allg = all_gather_fused(loc) if env.world_size > 1 else loc
    lab = labels + env.world_rank * labels.shape[0]
    ce = torch.nn.functional.cross_entropy
    tot = sum(ce(logit_scale * loc[a] @ allg[b].t(), lab) for a, b in ((0, 1), (1, 0), (3, 2), (2, 3), (0, 3), (1, 2)))
    return {"contrastive": tot, "total": tot}


def _toy_batch(n):
    g = torch.Generator().manual_seed(11)
    return {"images": torch.randn(n, 6, generator=g), "image_views": torch.randn(n, 6, generator=g),
            "text": torch.randn(n, 4, generator=g), "text2": torch.randn(n, 4, generator=g)}


def _w2_micro_worker(rank, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    sys.path.insert(0, ROOT)
    from mammo_clip_amd import engine
    from mammo_clip_amd.breastclip import util as U
    U.GlobalEnv.reset()
    full = _toy_batch(16)
    mine = {k: v[rank * 8:(rank + 1) * 8] for k, v in full.items()}
    m = _ToyClip()
    # bench.py's N = 8 policy: 4 micro-batches per rank, all four graphs kept, recompute mode 3 for the kept graphs, gradient
    # sink on, buckets all-reduced (AVG) after the last backward
    m.image_encoder.set_recompute(3)                  # (bench.py: model_cfg(..., recompute=3) -- every graph is a kept graph)
    tr = engine.Trainer(m, _toy_loss, torch.optim.SGD(m.parameters(), lr=0.0), None, None, bucket_mb=1, keep_graphs=4)
    out = tr.step(mine, micro_batches=4)
    ok = m.modes_seen == [(3, True)] * 4              # four forwards, all with a graph: no re-forward at all
    ok = ok and tr.buckets is not None and m.unused.grad is None
    ret[rank] = (bool(ok), float(out["total"]), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    dist.destroy_process_group()


def test_world2_micro_batched_step_with_all_graphs_kept_matches_single_process():
    """VERDICT r5 #7b: ``Trainer.step(batch, micro_batches=4)`` at world size 2 over gloo with ``keep_graphs=4`` and
    MBConv recompute mode 3 (the policy bench.py picks at N = 8: no re-forward) == the world-size-1 step over the concatenated
    batch cut into 8 micro-batches (one kept graph, seven re-forwards): mean over ranks of the per-rank loss, rank-averaged
    gradients of the global loss [ref: trainer_ddp.py:53-63,134; util/dist_autograd.py:5-27]."""
    import torch.multiprocessing as mp
    from mammo_clip_amd import engine
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_w2_micro_worker, args=(29741, ret), nprocs=2, join=True)
    (ok0, l0, g0), (ok1, l1, g1) = ret[0], ret[1]
    assert ok0 and ok1
    util.GlobalEnv.reset()
    m = _ToyClip()
    tr = engine.Trainer(m, _toy_loss, torch.optim.SGD(m.parameters(), lr=0.0), None, None, keep_graphs=1)
    out = tr.step(_toy_batch(16), micro_batches=8)
    assert [g for _, g in m.modes_seen] == [False] * 7 + [True] * 8          # 7 graph-less forwards, 1 kept, 7 re-forwards
    assert abs(float(out["total"]) - 0.5 * (l0 + l1)) < 1e-5
    for n, p in m.named_parameters():
        if p.grad is None:
            assert n not in g0
            continue
        assert torch.equal(g0[n], g1[n]), n                                   # all-reduced: identical on both ranks
        torch.testing.assert_close(g0[n], p.grad, rtol=2e-5, atol=2e-6)
