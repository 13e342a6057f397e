"""Worker of tests/test_eval_metrics_gpu.py: runs in a process of its own with MC_STORAGE=f16 (the storage type is fixed when
the kernel library is loaded) and prints ONE JSON line: the device-path metrics on the reference fixture."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _eval_common as E                                            # noqa: E402
from mammo_clip_amd import lib as L, ops                            # noqa: E402
from mammo_clip_amd.breastclip.evaluator import Evaluator           # noqa: E402

assert L.STORAGE == "f16" and ops.BF16 == torch.float16 and L.load().mc_storage_is_f16() == 1


def device_metrics(fx):
    dev = torch.device("cuda")
    out = {}
    for tag, c in fx["retrieval"].items():
        out[tag] = Evaluator.retrieval_i2t(torch.as_tensor(c["image"]).to(dev), torch.as_tensor(c["text"]).to(dev), c["texts"])
    z = fx["zs"]
    out["zs"] = Evaluator.zeroshot_metrics(torch.as_tensor(z["image"]).to(dev),
                                           {k: torch.as_tensor(v).to(dev) for k, v in z["prompts"].items()}, z["labels"])
    return out


if __name__ == "__main__":
    print("EVAL-F16-WORKER " + json.dumps(device_metrics(E.load())))
