"""Worker of tests/test_cls_metrics_gpu.py: runs in a process of its own with MC_STORAGE=f16 (the storage type is fixed when
the kernel library is loaded) and prints ONE JSON line: the device-path classification metrics on the reference fixture."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _cls_common as C                                             # noqa: E402
from mammo_clip_amd import lib as L, ops                            # noqa: E402
from mammo_clip_amd.breastclip import evaluator as EV               # noqa: E402

assert L.STORAGE == "f16" and ops.BF16 == torch.float16 and L.load().mc_storage_is_f16() == 1


def device_metrics(fx):
    dev = torch.device("cuda")
    out = {}
    for tag, c in fx["binary"].items():
        y, s = torch.as_tensor(c["label"]).to(dev), torch.as_tensor(c["score"]).to(dev)
        _, precision, recall = EV.pr_auc(y, s, get_all=True)
        out[tag] = dict(metrics=EV.binary_metrics(y, s, fx["threshold"]), precision=precision.tolist(), recall=recall.tolist(),
                        pfbeta=[EV.pfbeta(y, s, b) for b in fx["betas"]])
    z = fx["zs"]
    out["zs"] = EV.Evaluator.zeroshot_metrics(torch.as_tensor(z["image"]).to(dev),
                                              {k: torch.as_tensor(v).to(dev) for k, v in z["prompts"].items()}, z["labels"],
                                              detail=True)
    return out


if __name__ == "__main__":
    print("CLS-F16-WORKER " + json.dumps(device_metrics(C.load())))
