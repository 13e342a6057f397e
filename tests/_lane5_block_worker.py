"""Worker of tests/test_lane5_fused_gpu.py::test_block_backward_fused_against_two_launches: one 5x5 stride-1 MBConv block,
forward + backward, under the MC_DW_FUSED value of the environment (read once per process by the library).  Prints one line:
LANE5-BLOCK-WORKER {"fused_dw5": bool, "y": [...], "grads": {name: [...]}}"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
from mammo_clip_amd.breastclip.model.modules import efficientnet_custom as enc  # noqa: E402

DEV = torch.device("cuda:0")


def rnd(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV).to(ops.BF16)


def main():
    gp = enc.GlobalParams(1.0, 1.0, 224, 0.2, 1, 0.99, 1e-3, 0.2, 8, None, True)
    n, h, w, cin = 2, 24, 29, 48
    torch.manual_seed(5)
    blk = enc.MBConvBlock(enc.BlockArgs(1, 5, 1, 6, cin, cin, 0.25, True), gp, (h, w)).to(DEV)
    assert blk.args.pad == (2, 2, 2, 2), blk.args.pad
    with torch.no_grad():
        for nm, p_ in blk.named_parameters():
            if nm.endswith("_bn0.weight") or nm.endswith("_bn1.weight") or nm.endswith("_bn2.weight"):
                p_.copy_(1.0 + 0.2 * torch.randn_like(p_))
            elif nm.endswith(".bias"):
                p_.copy_(0.1 * torch.randn_like(p_))
    blk.train()
    xin = rnd(n * h * w, cin, seed=11).requires_grad_(True)
    y = blk(xin, n, h, w)
    fused_dw5 = bool(y.grad_fn.plan.fused_dw5)
    y.backward(rnd(n * h * w, cin, seed=12))
    torch.cuda.synchronize()
    grads = {k: p_.grad.detach().float().reshape(-1).cpu().tolist() for k, p_ in blk.named_parameters() if p_.grad is not None}
    grads["dx"] = xin.grad.detach().float().reshape(-1).cpu().tolist()
    print("LANE5-BLOCK-WORKER " + json.dumps({"fused_dw5": fused_dw5, "y": y.detach().float().reshape(-1).cpu().tolist(), "grads": grads}))


if __name__ == "__main__":
    main()
