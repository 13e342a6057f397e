#!/usr/bin/env python3
"""DEV-ONLY generator of tests/golden/mlp_head.npz.  Runs in the build container only (needs /root/reference).

Loads the REFERENCE's ``breastclip/model/modules/projection.py`` (it needs nothing but ``torch.nn``) from the reference tree,
builds ``MLPProjectionHead(40, 24, 0.1)`` in fp64 and eval mode with seeded weights (non-trivial LayerNorm gamma / beta and
biases), and stores what it computed on a seeded [5, 40] input: the output and the gradients of ``sum(out * cotangent)`` with
respect to the input and the six parameters.  Data only, a few KB; nothing of the reference travels.  (Train-mode dropout
uses torch's RNG there and cannot be matched: the masked path is tested against a host Philox mask instead.)

    python tests/golden/make_mlp_head_golden.py
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/codebase/breastclip/model/modules/projection.py"
EMB, N, ROWS, P = 40, 24, 5, 0.1


def main():
    spec = importlib.util.spec_from_file_location("ref_projection", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(20240611)

    def rnd(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift

    head = mod.MLPProjectionHead(EMB, N, P).double().eval()
    sd = {"projection.weight": rnd(N, EMB, scale=EMB ** -0.5), "projection.bias": rnd(N, scale=0.3),
          "fc.weight": rnd(N, N, scale=N ** -0.5), "fc.bias": rnd(N, scale=0.3),
          "layer_norm.weight": rnd(N, scale=0.25, shift=1.0), "layer_norm.bias": rnd(N, scale=0.2)}
    head.load_state_dict(sd, strict=True)
    x = rnd(ROWS, EMB).requires_grad_(True)
    cot = rnd(ROWS, N)
    out = head(x)
    (out * cot).sum().backward()
    z = {"meta": np.array([EMB, N, ROWS], dtype=np.int64), "x": x.detach().numpy(), "cotangent": cot.numpy(),
         "out": out.detach().numpy(), "grad/x": x.grad.numpy()}
    for k, v in head.named_parameters():
        z["w/" + k] = v.detach().numpy()
        z["grad/" + k] = v.grad.numpy()
    path = os.path.join(HERE, "mlp_head.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes", sorted(z))


if __name__ == "__main__":
    main()
