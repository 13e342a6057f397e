"""Worker of tests/test_mlp_head_gpu.py: runs in a process of its own with MC_STORAGE=f16 (the storage type is fixed when the
kernel library is loaded), takes ONE loss-scaled Trainer step of B2 + BERT-base with MLP projection heads and prints one JSON
line.  usage: python tests/_mlp_head_f16_worker.py"""
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _mlp_head_common as H                         # noqa: E402
from mammo_clip_amd import engine, lib as L, ops    # noqa: E402
from mammo_clip_amd.breastclip import util          # noqa: E402
from mammo_clip_amd.breastclip.loss import build_loss              # noqa: E402
from mammo_clip_amd.breastclip.model import build_model            # noqa: E402
from mammo_clip_amd.breastclip.optimizer import build_optimizer    # noqa: E402
from oracle import weights as ow                    # noqa: E402

assert L.STORAGE == "f16" and ops.BF16 == torch.float16 and L.load().mc_storage_is_f16() == 1
DEV = torch.device("cuda:0")


def main():
    model = build_model(H.cfg("mlp"), H.LOSS_CFG, types.SimpleNamespace(vocab_size=28996))
    sd = H.mlp_state_dict()
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    batch = ow.synth_batch(4, 160, 96, 32, seed=21)
    bt = {"images": batch["images"].to(DEV), "image_views": batch["image_views"].to(DEV),
          "text_tokens": {k: v.to(DEV) for k, v in batch["text_tokens"].items()},
          "text_tokens2": {k: v.to(DEV) for k, v in batch["text_tokens2"].items()}}
    util.GlobalEnv.reset()
    opt = build_optimizer(model, {"name": "adamw", "config": {"lr": 1e-4, "weight_decay": 1e-4}})
    tr = engine.Trainer(model, build_loss(H.LOSS_CFG), opt, None, DEV)
    rep = {"scaler": type(tr.scaler).__name__}
    tr.scaler = engine.LossScaler(init_scale=256.0)           # low enough not to overflow f16 on this small model
    out = tr.step(bt)
    heads = [(f"{h}.{k}", v) for h in ("image_projection", "text_projection") for k, v in getattr(model, h).named_parameters()]
    rep["loss_finite"] = bool(torch.isfinite(out["total"]).all())
    rep["skipped"] = tr.scaler.skipped
    rep["head_params"] = len(heads)
    rep["head_grads_finite_nonzero"] = sum(int(p.grad is not None and bool(torch.isfinite(p.grad).all())
                                               and float(p.grad.abs().max()) > 0) for _, p in heads)
    rep["head_params_changed"] = sum(int(not torch.equal(p.detach().cpu(), sd[n])) for n, p in heads)
    print("MLP-F16 " + json.dumps(rep))


if __name__ == "__main__":
    main()
