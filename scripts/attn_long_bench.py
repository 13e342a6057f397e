"""Developer measurement: the long fused attention kernels (mc_attn_long_*, 257..512 keys) against the unfused path they replace
(batched GEMM -> fp32 scores -> mc_softmax_fwd -> batched GEMM, and its backward), on the same operands.

    timeout 900 python scripts/attn_long_bench.py [--b 32] [--nh 12] [--Ts 512,320] [--p 0.1] [--rounds 7] [--iters 200]

One process.  Per T: seeded N(0, 1.5) qkv and N(0, 1) dctx, ragged prefix masks; both routes are warmed up, their outputs are
compared (same seed = same dropout masks: max-abs difference relative to max|ref| of ctx and dqkv), then long and unfused rounds
ALTERNATE and each round is timed with device events around ``iters`` forward + backward passes of the attention core alone;
median and min per pass over the rounds are reported.  Then the peak allocated memory (torch.cuda.max_memory_allocated above
what is resident before the pass) of one forward + backward of a 12-layer BERT-base encoder at [b, max(Ts)] tokens, train mode,
on both routes (MC_FUSED_ATTN=0 selects the unfused one).  Prints one JSON object per measurement; not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd import ops  # noqa: E402
from mammo_clip_amd.breastclip.model.modules.text_encoder import BertConfigLite, BertModelHIP  # noqa: E402


def long_pass(qkv, maskb, dctx, b, t, nh, p, seed, sid):
    ctx, lse = ops.attn_long_fwd(qkv, maskb, b, t, nh, 0.125, p, seed, sid)
    return ctx, ops.attn_long_bwd(qkv, maskb, dctx, lse, b, t, nh, 0.125, p, seed, sid)


def unfused_pass(qkv, maskb, dctx, b, t, nh, p, seed, sid):
    """the attention core of _LayerFn's unfused path, forward and backward"""
    H, M, hd, dev = nh * 64, b * t, 64, qkv.device
    scores = torch.empty((b, nh, t, t), dtype=torch.float32, device=dev)
    ops.gemm(qkv, qkv[:, H:], scores, t, t, hd, 3 * H, 3 * H, t, c_f32=1, batch=b * nh, nb2=nh,
             sA=(t * 3 * H, hd), sB=(t * 3 * H, hd), sC=(nh * t * t, t * t), bias=maskb, bias_stride1=t, alpha=0.125)
    probs, pd = ops.softmax_fwd(scores, p, seed, sid)
    del scores
    ctx = torch.empty((M, H), dtype=ops.BF16, device=dev)
    ops.gemm(pd, qkv[:, 2 * H:], ctx, t, hd, t, t, 3 * H, H, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * H, hd))
    dpd = torch.empty((b, nh, t, t), dtype=torch.float32, device=dev)
    ops.gemm(dctx, qkv[:, 2 * H:], dpd, t, t, hd, H, 3 * H, t, c_f32=1, batch=b * nh, nb2=nh,
             sA=(t * H, hd), sB=(t * 3 * H, hd), sC=(nh * t * t, t * t))
    dqkv = torch.empty((M, 3 * H), dtype=ops.BF16, device=dev)
    ops.gemm(pd, dctx, dqkv[:, 2 * H:], t, hd, t, t, H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * H, hd), sC=(t * 3 * H, hd))
    ds = ops.softmax_bwd(probs, dpd, p, seed, sid, 0.125)
    del dpd
    ops.gemm(ds, qkv[:, H:], dqkv, t, hd, t, t, 3 * H, 3 * H, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * 3 * H, hd))
    ops.gemm(ds, qkv, dqkv[:, H:], t, hd, t, t, 3 * H, 3 * H, a_kmajor=1, b_kmajor=1, batch=b * nh, nb2=nh,
             sA=(nh * t * t, t * t), sB=(t * 3 * H, hd), sC=(t * 3 * H, hd))
    return ctx, dqkv


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def prefix_mask(b, t, gen):
    ln = torch.randint(t // 2, t + 1, (b,), generator=gen)
    ln[0] = t
    return (torch.arange(t)[None, :] < ln[:, None]).long()


def core_times(args, t, dev, gen):
    b, nh, H, p, seed, sid = args.b, args.nh, args.nh * 64, args.p, 1234, 16
    qkv = (torch.randn((b * t, 3 * H), generator=gen) * 1.5).to(dev).to(ops.BF16)
    dctx = torch.randn((b * t, H), generator=gen).to(dev).to(ops.BF16)
    maskb = ops.mask_bias(prefix_mask(b, t, gen).to(dev))
    routes = {"long": long_pass, "unfused": unfused_pass}
    out = {}
    for name, fn in routes.items():                        # warm-up of every shape of the timed window
        for _ in range(3):
            out[name] = fn(qkv, maskb, dctx, b, t, nh, p, seed, sid)
    torch.cuda.synchronize()
    row = {"what": "attention core fwd+bwd", "b": b, "T": t, "nh": nh, "p": p,
           "ctx_long_vs_unfused": rel(out["long"][0], out["unfused"][0]), "dqkv_long_vs_unfused": rel(out["long"][1], out["unfused"][1])}
    del out
    ms = {name: [] for name in routes}
    for _ in range(args.rounds):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn(qkv, maskb, dctx, b, t, nh, p, seed, sid)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.iters)
    for name in routes:
        row[name + "_ms_median"], row[name + "_ms_min"], row[name + "_ms_max"] = statistics.median(ms[name]), min(ms[name]), max(ms[name])
    row["unfused_over_long"] = row["unfused_ms_median"] / row["long_ms_median"]
    return row


def encoder_peaks(args, t, dev, gen):
    torch.manual_seed(1234)
    model = BertModelHIP(BertConfigLite()).to(dev).train()
    b = args.b
    mask = prefix_mask(b, t, gen)
    ids = torch.randint(1000, 28996, (b, t), generator=gen) * mask
    tok = {"input_ids": ids.to(dev), "attention_mask": mask.to(dev), "token_type_ids": torch.zeros_like(ids).to(dev)}
    r = torch.randn((b, t, 768), generator=gen).to(dev)
    row = {"what": "12-layer BERT-base fwd+bwd, peak allocated above the resident state", "b": b, "T": t}
    old = os.environ.get("MC_FUSED_ATTN")
    try:
        for name, switch in (("long", "1"), ("unfused", "0")):
            os.environ["MC_FUSED_ATTN"] = switch

            def one_pass():
                model.zero_grad(set_to_none=True)
                (model(**tok)["last_hidden_state"].float() * r).sum().backward()
            one_pass()
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            one_pass()
            torch.cuda.synchronize()
            row[name + "_peak_bytes"] = torch.cuda.max_memory_allocated() - base
            row[name + "_peak_mib"] = row[name + "_peak_bytes"] / 2 ** 20
    finally:
        if old is None:
            os.environ.pop("MC_FUSED_ATTN", None)
        else:
            os.environ["MC_FUSED_ATTN"] = old
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--nh", type=int, default=12)
    ap.add_argument("--Ts", default="512,320")
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-encoder", action="store_true", help="skip the encoder memory measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to measure on a CPU")
    if os.environ.get("MC_FUSED_ATTN", "1") == "0":
        raise SystemExit("MC_FUSED_ATTN=0 is set: the long route is switched off")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1234)
    ts = [int(v) for v in args.Ts.split(",")]
    for t in ts:
        if not ops.attn_long_supported(t, 64):
            raise SystemExit(f"T = {t}: not a shape of the long kernels")
        print(json.dumps(core_times(args, t, dev, gen)), flush=True)
    if not args.no_encoder:
        print(json.dumps(encoder_peaks(args, max(ts), dev, gen)), flush=True)


if __name__ == "__main__":
    main()
