"""RCCL smoke of the data-parallel exchange steps on ONE GPU (world_size 1, backend "nccl" = RCCL): the collectives the
multi-GPU run issues -- fused embedding all-gather / reduce-scatter [ref: util/dist_autograd.py:5-27], bucketed
gradient all-reduce(AVG) from post-accumulate hooks [ref: trainer_ddp.py:134 DDP], validation loss all-reduce
[ref: trainer_ddp.py:384-387] -- run through the real backend with GPU tensors, and a full Trainer.step with the
buckets forced on matches the plain single-process step.  (Rank arithmetic is covered by the world_size-2 gloo tests.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, types
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%s" % sys.argv[2], rank=0, world_size=1, device_id=dev)
import mammo_clip_amd
from mammo_clip_amd import engine
from mammo_clip_amd.breastclip import util as U
from mammo_clip_amd.breastclip.util.dist_autograd import all_gather_fused, DistAutogradAllGatherFunction
from mammo_clip_amd.breastclip.loss import build_loss
from mammo_clip_amd.breastclip.model import build_model
from mammo_clip_amd.breastclip.optimizer import build_optimizer
from oracle import weights as ow

# the exchange steps are ONE code path for every backend: count the torch.distributed entry points RCCL is given here --
# the world-size-2 gloo tests (tests/test_host_cpu.py, below) assert the same names
calls = {"all_gather_into_tensor": 0, "reduce_scatter_tensor": 0, "all_reduce_avg": 0}
_ag, _rs, _ar = dist.all_gather_into_tensor, dist.reduce_scatter_tensor, dist.all_reduce
def ag(*a_, **k_): calls["all_gather_into_tensor"] += 1; return _ag(*a_, **k_)
def rs(*a_, **k_): calls["reduce_scatter_tensor"] += 1; return _rs(*a_, **k_)
def ar(t_, op=dist.ReduceOp.SUM, **k_):
    calls["all_reduce_avg"] += int(op == dist.ReduceOp.AVG); return _ar(t_, op=op, **k_)
dist.all_gather_into_tensor, dist.reduce_scatter_tensor, dist.all_reduce = ag, rs, ar
dist.all_gather = dist.reduce_scatter = None          # the list forms are not part of the product path any more

# 1. fused gather / reduce-scatter and the reference-style per-tensor function on RCCL
a = torch.randn(5, 512, device=dev, requires_grad=True); b = torch.randn(5, 512, device=dev, requires_grad=True)
ga, gb = all_gather_fused([a, b])
assert torch.equal(ga, a) and torch.equal(gb, b)
(ga * 2).sum().backward(retain_graph=True); (gb * 3).sum().backward()
assert torch.equal(a.grad, torch.full_like(a, 2.0)) and torch.equal(b.grad, torch.full_like(b, 3.0))
t = torch.randn(4, 8, device=dev, requires_grad=True)
(out,) = DistAutogradAllGatherFunction(partial=False).apply(t)
out.sum().backward()
assert torch.equal(out, t) and torch.equal(t.grad, torch.ones_like(t))
assert calls["all_gather_into_tensor"] == 2 and calls["reduce_scatter_tensor"] == 3, calls    # (retain_graph: two backward calls)

# 2. one training step with the gradient buckets forced on == the plain step (AVG over one rank is the identity)
cfg = {"name": "clip_custom", "temperature": 0.07,
       "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": False, "model_type": "cnn"},
       "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                        "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
       "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
batch = ow.synth_batch(2, 64, 64, 16, seed=3)
bt = {"images": batch["images"].to(dev), "image_views": batch["image_views"].to(dev),
      "text_tokens": {k: v.to(dev) for k, v in batch["text_tokens"].items()},
      "text_tokens2": {k: v.to(dev) for k, v in batch["text_tokens2"].items()}}
res = []
for buckets in (False, True):
    torch.manual_seed(0)
    U.GlobalEnv.reset()
    model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996)).to(dev)
    opt = build_optimizer(model, {"name": "adamw", "config": {"lr": 1e-4, "weight_decay": 1e-4}})
    tr = engine.Trainer(model, build_loss(loss_cfg), opt, None, dev, bucket_mb=16)
    if buckets:
        tr.buckets = engine.GradBuckets(list(model.parameters()), 16 << 20)
        assert len(tr.buckets.buckets) > 3
    losses = [float(tr.step(bt)["total"]) for _ in range(2)]
    res.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
(l0, s0), (l1, s1) = res
assert l0[0] == l1[0], (l0, l1)
assert abs(l0[1] - l1[1]) < 5e-3, (l0, l1)        # float atomics in the depthwise weight gradient: round-off only
worst = max(float((s0[k].float() - s1[k].float()).abs().max()) for k in s0)
assert worst < 5e-3, worst
assert calls["all_reduce_avg"] == 2 * len(tr.buckets.buckets), calls      # every bucket of both steps went through all_reduce(AVG)

# 3. validation: one all-reduce per batch on the device
out = engine.validate(model, build_loss(loss_cfg), {"v": [bt, bt]}, dev)
assert abs(out["v"]["total"] - out["v"]["contrastive"]) < 1e-6 and out["v"]["total"] > 0
dist.destroy_process_group()
print("RCCL-OK")
'''


@pytest.mark.gpu
def test_rccl_world1_exchange_steps(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(WORKER)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), ROOT, "29877"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "RCCL-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


WORKER2 = r'''
import os, sys, types
sys.path.insert(0, sys.argv[1])
rank, port, outdir = int(sys.argv[2]), sys.argv[3], sys.argv[4]
backend = sys.argv[5] if len(sys.argv) > 5 else "gloo"          # "nccl" = RCCL, one GPU per rank
micro = int(sys.argv[6]) if len(sys.argv) > 6 else 1
overlap = (int(sys.argv[7]) if len(sys.argv) > 7 else 1) != 0
keep = int(sys.argv[8]) if len(sys.argv) > 8 else 1              # kept graphs of the micro-batched step
recompute = int(sys.argv[9]) if len(sys.argv) > 9 else 0         # MBConv recompute mode of the model
import torch, torch.distributed as dist
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
dev = torch.device("cuda:%d" % (rank if backend == "nccl" else 0)); torch.cuda.set_device(dev)
if backend == "nccl":
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%s" % port, rank=rank, world_size=2, device_id=dev)
else:
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % port, rank=rank, world_size=2)
import mammo_clip_amd
from mammo_clip_amd import engine
from mammo_clip_amd.breastclip import util as U
from mammo_clip_amd.breastclip.loss import build_loss
from mammo_clip_amd.breastclip.model import build_model
from oracle import weights as ow
cfg = {"name": "clip_custom", "temperature": 0.07,
       "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": False, "model_type": "cnn"},
       "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                        "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
       "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
U.GlobalEnv.reset()
assert U.GlobalEnv.get().world_size == 2
torch.manual_seed(0)
model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996)).to(dev)
per = 2 * micro                                     # pairs per rank
batch = ow.synth_batch(2 * per, 64, 64, 16, seed=5)
lo, hi = rank * per, rank * per + per
bt = {"images": batch["images"][lo:hi].to(dev), "image_views": batch["image_views"][lo:hi].to(dev),
      "text_tokens": {k: v[lo:hi].to(dev) for k, v in batch["text_tokens"].items()},
      "text_tokens2": {k: v[lo:hi].to(dev) for k, v in batch["text_tokens2"].items()}}
# the second rank replays the seeds the second MICRO-batch of the single-process run gets (2 image-encoder calls and ONE
# text-encoder call -- both reports of a pair go through BERT together -- per micro-batch)
# (with micro > 1 the micro-batched step forwards every micro-batch twice: first pass + replay, so the single-process
# reference below cannot share seeds -- those runs switch dropout / drop-connect off instead)
model.image_encoder.rng.calls = 2 * rank
model.text_encoder.text_encoder._calls = rank * (1 if os.environ.get("MC_TEXT_ONE_CALL", "1") != "0" else 2)
if micro > 1:
    enc = model.image_encoder
    enc._dropout_p = 0.0
    enc._global_params = enc._global_params._replace(drop_connect_rate=0.0)
    for lyr in model.text_encoder.text_encoder.encoder.layer:
        lyr.p_attn = lyr.p_hidden = 0.0
    model.text_encoder.text_encoder.config.hidden_dropout_prob = 0.0
if recompute:
    model.image_encoder.set_recompute(recompute)
tr = engine.Trainer(model, build_loss(loss_cfg), torch.optim.SGD(model.parameters(), lr=0.0), None, dev, bucket_mb=16,
                    overlap_micro=overlap, grad_sink=not overlap, keep_graphs=keep)    # overlapped hooks <-> plain autograd accumulation; serial <-> sink
assert tr.buckets is not None and len(tr.buckets.buckets) > 3
out = tr.step(bt, micro_batches=micro)
torch.save({"loss": float(out["total"]), "grads": {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}},
           os.path.join(outdir, "r%d.pt" % rank))
dist.destroy_process_group()
print("DP-OK")
'''


@pytest.mark.gpu
def test_two_rank_step_equals_micro_batched_single_process(tmp_path):
    """Data-parallel identity on the real model (2 processes sharing the one GPU, gloo): mean over ranks of the per-rank
    loss == loss over the concatenated batch, and the bucket-averaged gradients == the gradients of that global loss
    with per-rank BatchNorm statistics -- which is what the single-process micro-batched step computes (k = 2)."""
    import torch
    import types
    script = tmp_path / "w2.py"
    script.write_text(WORKER2)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    # (the ranks run plain single-pass steps: recompute mode 1 makes them take the fused expand + depthwise forward the
    # micro-batched single-process step takes -- at 64 x 64 pixels BatchNorm over a handful of samples amplifies the one
    # 16-bit rounding the two forward forms differ by to tens of per cent in the last stages)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), "29879", str(tmp_path), "gloo", "1", "1", "1", "1"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    assert all(p.returncode == 0 and "DP-OK" in o[0] for p, o in zip(procs, outs)), [o[1][-3000:] for o in outs]
    r0, r1 = (torch.load(tmp_path / ("r%d.pt" % r)) for r in range(2))
    for n in r0["grads"]:
        assert torch.equal(r0["grads"][n], r1["grads"][n]), n            # all-reduced: identical on both ranks

    sys.path.insert(0, ROOT)
    import mammo_clip_amd  # noqa: F401
    from mammo_clip_amd import engine
    from mammo_clip_amd.breastclip import util as U
    from mammo_clip_amd.breastclip.loss import build_loss
    from mammo_clip_amd.breastclip.model import build_model
    from oracle import weights as ow
    dev = torch.device("cuda:0")
    cfg = {"name": "clip_custom", "temperature": 0.07,
           "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": False, "model_type": "cnn"},
           "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                            "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
           "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
    loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
    U.GlobalEnv.reset()
    torch.manual_seed(0)
    model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996)).to(dev)
    batch = ow.synth_batch(4, 64, 64, 16, seed=5)
    bt = {"images": batch["images"].to(dev), "image_views": batch["image_views"].to(dev),
          "text_tokens": {k: v.to(dev) for k, v in batch["text_tokens"].items()},
          "text_tokens2": {k: v.to(dev) for k, v in batch["text_tokens2"].items()}}
    tr = engine.Trainer(model, build_loss(loss_cfg), torch.optim.SGD(model.parameters(), lr=0.0), None, dev)
    out = tr.step(bt, micro_batches=2)
    # Same forward bit for bit (same counter-based dropout seeds), same loss; the embedding gradients differ in their fp32
    # summation order (two 2-row partial sums reduce-scattered vs one 4-row sum: ~1e-7 relative), and with BatchNorm over
    # two images of up to 2x2 pixels a single bf16 rounding flip grows to per cents on individual early-layer elements
    # (scripts/dbg_proc.py: a 1e-7 perturbation of d loss / d embeddings alone moves 242 of 501 parameter gradients by
    # more than 5e-3 of their max) -- so: loss identity, and direction / length of the whole gradient
    ref_g = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
    for n in r0["grads"]:
        assert n in ref_g or float(r0["grads"][n].abs().max()) == 0.0, n
    _check_against_reference(r0, r1, float(out["total"]), ref_g, tol=None)


def _single_process_reference(n_pairs, k, stochastic_off):
    import torch
    import types
    sys.path.insert(0, ROOT)
    import mammo_clip_amd  # noqa: F401
    from mammo_clip_amd import engine
    from mammo_clip_amd.breastclip import util as U
    from mammo_clip_amd.breastclip.loss import build_loss
    from mammo_clip_amd.breastclip.model import build_model
    from oracle import weights as ow
    dev = torch.device("cuda:0")
    cfg = {"name": "clip_custom", "temperature": 0.07,
           "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": False, "model_type": "cnn"},
           "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                            "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
           "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
    loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
    U.GlobalEnv.reset()
    torch.manual_seed(0)
    model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996)).to(dev)
    if stochastic_off:
        enc = model.image_encoder
        enc._dropout_p = 0.0
        enc._global_params = enc._global_params._replace(drop_connect_rate=0.0)
        for lyr in model.text_encoder.text_encoder.encoder.layer:
            lyr.p_attn = lyr.p_hidden = 0.0
        model.text_encoder.text_encoder.config.hidden_dropout_prob = 0.0
    batch = ow.synth_batch(n_pairs, 64, 64, 16, seed=5)
    bt = {"images": batch["images"].to(dev), "image_views": batch["image_views"].to(dev),
          "text_tokens": {kk: v.to(dev) for kk, v in batch["text_tokens"].items()},
          "text_tokens2": {kk: v.to(dev) for kk, v in batch["text_tokens2"].items()}}
    tr = engine.Trainer(model, build_loss(loss_cfg), torch.optim.SGD(model.parameters(), lr=0.0), None, dev)
    out = tr.step(bt, micro_batches=k)
    return float(out["total"]), {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}


def _run_two_ranks(tmp_path, port, backend, micro, overlap=1, keep=1, recompute=0):
    script = tmp_path / "w2.py"
    script.write_text(WORKER2)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), str(port), str(tmp_path), backend, str(micro), str(overlap),
                               str(keep), str(recompute)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(2)]
    outs = [p.communicate(timeout=900) for p in procs]
    assert all(p.returncode == 0 and "DP-OK" in o[0] for p, o in zip(procs, outs)), [o[1][-3000:] for o in outs]
    import torch
    return [torch.load(tmp_path / ("r%d.pt" % r)) for r in range(2)]


def _check_against_reference(r0, r1, ref_loss, ref_g, tol=5e-3):
    """tol: max-abs deviation relative to the tensor's max (None: direction / length criteria only -- used where the two
    runs differ in the fp32 summation order of the embedding gradients and BatchNorm over a handful of samples amplifies
    single bf16 rounding flips to several per cent on individual early-layer elements)"""
    import torch
    for n in r0["grads"]:
        assert torch.equal(r0["grads"][n], r1["grads"][n]), n            # all-reduced: identical on both ranks
    assert abs(ref_loss - 0.5 * (r0["loss"] + r1["loss"])) < 1e-5
    worst, dots = ("", 0.0), [0.0, 0.0, 0.0]
    for n, g in ref_g.items():
        h = r0["grads"][n]
        e = float((g - h).abs().max() / (g.abs().max() + 1e-12))
        worst = max(worst, (n, e), key=lambda t: t[1])
        if tol is not None:
            assert e < tol, (n, e)
        gd, hd = g.double().reshape(-1), h.double().reshape(-1)
        dots[0] += float(gd @ hd); dots[1] += float(gd @ gd); dots[2] += float(hd @ hd)
        if tol is not None and float(gd.norm()) > 1e-6:
            c = float(gd @ hd / (gd.norm() * hd.norm() + 1e-300))
            assert c > 0.98 and abs(float(hd.norm() / gd.norm()) - 1.0) < 0.05, (n, c)
    cos_all = dots[0] / (dots[1] * dots[2]) ** 0.5
    print("worst element deviation vs the single-process step:", worst, "cosine over all gradients:", cos_all)
    assert cos_all > 0.999 and abs((dots[2] / dots[1]) ** 0.5 - 1.0) < 0.02, cos_all


@pytest.mark.gpu
def test_two_rank_micro_batched_step_overlapped_buckets(tmp_path):
    """The cfg4 mode: every rank runs a MICRO-BATCHED step (k = 2) and the gradient buckets are all-reduced from the
    hooks of the last micro-batch's backward (engine._step_micro).  2 ranks on the one GPU over gloo == the
    single-process micro-batched step with k = 4 over the concatenated batch (dropout / drop-connect off)."""
    import torch
    r0, r1 = _run_two_ranks(tmp_path, 29881, "gloo", 2, overlap=1)
    s0, s1 = _run_two_ranks(tmp_path, 29887, "gloo", 2, overlap=0)       # buckets reduced after the last backward
    # the overlapped and the serial form move the same accumulated gradients through the same collectives: every
    # gradient whose kernels are free of float atomics must come out BIT-identical (atomics: depthwise taps, embedding
    # rows, LayerNorm / BatchNorm-free scatter sums -- those are compared to round-off)
    det = ("_conv_stem.weight", "_expand_conv.weight", "_project_conv.weight", "_conv_head.weight", "projection.weight",
           "_bn0.weight", "_bn2.bias", "attention.self.query.weight", "intermediate.dense.weight", "logit_scale")
    for n, g in r0["grads"].items():
        if any(t in n for t in det):
            assert torch.equal(g, s0["grads"][n]), n
        else:
            assert float((g - s0["grads"][n]).abs().max()) <= 1e-3 * float(g.abs().max() + 1e-12), n
    assert r0["loss"] == s0["loss"] and r1["loss"] == s1["loss"]
    # against the single-process step over the concatenated batch: per-rank vs global summation order of the embedding
    # gradients differs in the last fp32 bit, and BatchNorm over 8 samples per channel (2 images of 2x2 pixels in the
    # last stages at this test size) amplifies that: a few per cent on the deepest layers
    ref_loss, ref_g = _single_process_reference(8, 4, True)
    _check_against_reference(r0, r1, ref_loss, ref_g, tol=None)


@pytest.mark.gpu
def test_two_rank_kept_graphs_recompute3_is_the_n8_policy(tmp_path):
    """The policy bench.py picks for the 8-GPU point of the headline workload (bench.py: 128 pairs per GPU = 4 micro-batches,
    ALL FOUR graphs kept in MBConv recompute mode 3, gradient sink, buckets reduced after the last backward) at world size 2
    over gloo == the single-process step over the concatenated batch with 8 micro-batches (one kept graph, 7 re-forwards,
    mode 0): same loss, same averaged gradients -- the kept-graph / recompute path changes what is stored, not what is
    computed [ref: trainer_ddp.py:53-63,134; util/dist_autograd.py:5-27]."""
    r0, r1 = _run_two_ranks(tmp_path, 29893, "gloo", 4, overlap=0, keep=4, recompute=3)
    ref_loss, ref_g = _single_process_reference(16, 8, True)
    _check_against_reference(r0, r1, ref_loss, ref_g, tol=None)


@pytest.mark.gpu
def test_two_rank_step_over_rccl(tmp_path):
    """RCCL with MORE than one rank (needs >= 2 GPUs; skipped on a 1-GPU box): fused embedding all-gather /
    reduce-scatter [ref: util/dist_autograd.py:5-27] and bucketed gradient all-reduce(AVG) [ref: trainer_ddp.py:134] over
    backend "nccl", one GPU per rank; plain step and micro-batched step, both against the single-process
    micro-batched step over the concatenated batch."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (RCCL refuses two ranks on one device)")
    r0, r1 = _run_two_ranks(tmp_path, 29883, "nccl", 1)
    ref_loss, ref_g = _single_process_reference(4, 2, False)
    _check_against_reference(r0, r1, ref_loss, ref_g)
    r0, r1 = _run_two_ranks(tmp_path, 29885, "nccl", 2)
    ref_loss, ref_g = _single_process_reference(8, 4, True)
    _check_against_reference(r0, r1, ref_loss, ref_g, tol=None)


WORKER_DDP = r'''
import os, sys, types
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%s" % sys.argv[2], rank=0, world_size=1, device_id=dev)
import mammo_clip_amd
from mammo_clip_amd.breastclip import util as U
from mammo_clip_amd.breastclip.loss import build_loss
from mammo_clip_amd.breastclip.model import build_model
from mammo_clip_amd.breastclip.optimizer import build_optimizer
from oracle import weights as ow
cfg = {"name": "clip_custom", "temperature": 0.07,
       "image_encoder": {"source": "cnn", "name": "tf_efficientnetv2-detect", "pretrained": False, "model_type": "cnn"},
       "text_encoder": {"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                        "gradient_checkpointing": False, "pooling": "eos", "cache_dir": "", "trust_remote_code": True},
       "projection_head": {"name": "linear", "dropout": 0.1, "proj_dim": 512}}
loss_cfg = {"breast_clip": dict(label_smoothing=0.0, i2i_weight=1.0, t2t_weight=0.5, loss_ratio=1.0)}
batch = ow.synth_batch(2, 64, 64, 16, seed=3)
bt = {"images": batch["images"].to(dev), "image_views": batch["image_views"].to(dev),
      "text_tokens": {k: v.to(dev) for k, v in batch["text_tokens"].items()},
      "text_tokens2": {k: v.to(dev) for k, v in batch["text_tokens2"].items()}}
res = []
for wrap in (False, True):
    torch.manual_seed(0)
    U.GlobalEnv.reset()
    model = build_model(cfg, loss_cfg, types.SimpleNamespace(vocab_size=28996)).to(dev)
    # exactly how the reference wraps it [ref: trainer_ddp.py:134]
    net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[0], find_unused_parameters=True) if wrap else model
    loss_func = build_loss(loss_cfg)
    opt = build_optimizer(net, {"name": "adamw", "config": {"lr": 1e-4, "weight_decay": 1e-4}})
    losses = []
    for step in range(2):                      # the reference's hot loop [ref: trainer_ddp.py:279-308]
        opt.zero_grad(set_to_none=True)
        net.train()
        out = net(bt, dev)
        ld = loss_func(**out, is_train=True)
        ld["total"].backward()
        opt.step()
        losses.append(float(ld["total"]))
    sd = {k.replace("module.", ""): v.detach().clone() for k, v in net.state_dict().items()}
    pooler = dict(model.named_parameters())["text_encoder.text_encoder.pooler.dense.weight"].grad
    assert pooler is None or float(pooler.abs().max()) == 0.0          # unused parameter: tolerated by find_unused_parameters
    res.append((losses, sd))
(l0, s0), (l1, s1) = res
assert l0[0] == l1[0], (l0, l1)
assert abs(l0[1] - l1[1]) < 5e-3, (l0, l1)
worst = max(float((s0[k].float() - s1[k].float()).abs().max()) for k in s0)
assert worst < 5e-3, worst
dist.destroy_process_group()
print("DDP-OK", l0, l1, worst)
'''


@pytest.mark.gpu
def test_model_under_torch_ddp_find_unused_parameters(tmp_path):
    """INTEGRATION.md claim: the model drops into the reference's trainer unchanged -- wrapped in torch's
    DistributedDataParallel(find_unused_parameters=True) [ref: trainer_ddp.py:134] over RCCL (world size 1 here), two
    steps of the reference's loop order with the HIP AdamW give the same losses and parameters as the unwrapped model."""
    script = tmp_path / "ddp.py"
    script.write_text(WORKER_DDP)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), ROOT, "29889"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "DDP-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.gpu
def test_bench_launches_two_ranks_and_prints_one_json_line():
    """``python bench.py --gpus 2`` end to end on a 1-GPU box: bench.py re-executes itself under torch.distributed.run on
    127.0.0.1, both ranks share the GPU over gloo (MC_DIST_BACKEND: RCCL refuses two ranks on one device), parameters are
    broadcast, the fused embedding gather / reduce-scatter and the bucketed gradient mean run with world size 2, and rank 0
    prints exactly one JSON line with n_gpus = 2 [ref: trainer_ddp.py:53-63,132-134]."""
    import json
    env = dict(os.environ, MC_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg1", "--steps", "1",
                        "--warmup", "1", "--no-cpu-baseline", "--full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    js = json.loads(lines[0])
    assert js["n_gpus"] == 2 and js["steps"] == 1 and js["value"] > 0 and js["config"]["global_batch"] == 8
    assert js["scaling"] == "weak" and js["roofline"] is not None and "cpu_baseline" not in js
    # the line says which backend the job's collectives ran on and how many ranks took part in one (round 5; over RCCL
    # "rccl_ranks" additionally carries the rank count RCCL's own INIT log reports -- gloo has no such log: None here)
    assert js["dist"]["backend"] == "gloo" and js["dist"]["allreduce_of_ones"] == 2 and js["rccl_ranks"] is None, js["dist"]


@pytest.mark.gpu
def test_bench_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain ``python bench.py --gpus 1`` run does only the headline: the contract fields, no --full objects (roofline,
    whole_step, parity, cpu_baseline); --dump-outputs writes the last timed step's loss terms and the parameter sample as
    float32 .npy files within 64 MB, and the dumped total loss is the one the line reports."""
    import json

    import numpy as np
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    js = json.loads(lines[0])
    assert js["steps"] == 3 and js["warmup"] == 1 and js["value"] > 0 and js["ms_per_step"] > 0 and js["higher_is_better"] is True
    assert abs(js["value"] - js["config"]["global_batch"] / (js["ms_per_step"] * 1e-3)) <= 1e-2 * js["value"]
    for k in ("roofline", "whole_step", "parity", "parity_build", "cpu_baseline", "n8_load", "dist"):
        assert k not in js, k
    files = sorted(p.name for p in out.iterdir())
    assert {"loss_total.npy", "params_sample.npy"} <= set(files), files
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
    arrs = {f: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
    assert abs(float(arrs["loss_total.npy"][0]) - js["config"]["loss"]) <= 1e-4
