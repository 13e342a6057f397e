"""Worker of tests/test_boot_metrics_gpu.py: runs in a process of its own with MC_STORAGE=f16 (the storage type is fixed when
the kernel library is loaded) and prints ONE JSON line: the device bootstrap records of the cases ``_boot_common.F16_CASES``."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _boot_common as B                                            # noqa: E402
import _cls_common as C                                             # noqa: E402
from mammo_clip_amd import lib as L, ops                            # noqa: E402

assert L.STORAGE == "f16" and ops.BF16 == torch.float16 and L.load().mc_storage_is_f16() == 1


def device_records():
    dev = torch.device("cuda")
    out = {}
    for n, kind, stratified in B.F16_CASES:
        score, label = C.kernel_case(n, kind)
        ds, dl = torch.as_tensor(np.ascontiguousarray(score)).to(dev), torch.as_tensor(label).to(dev)
        records = ops.boot_records(ds, dl, ops.rank_counts(ds, dl), B.F16_REPLICATES, B.THRESHOLD, B.SEED, stratified)
        out[f"{n}/{kind}/{int(stratified)}"] = records.cpu().numpy().tolist()
    return out


if __name__ == "__main__":
    print("BOOT-F16-WORKER " + json.dumps(device_records()))
