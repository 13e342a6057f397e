"""Developer measurement: the text tower (BERT-base, eos pooling) forward + backward, padded against packed
(BertModelHIP.set_packed), on synthetic prefix masks of a given fill = sum(len) / (n * T).

    timeout 900 python scripts/text_packed_bench.py [--seqs 128] [--T 256] [--fills 1.0,0.5,0.25,0.1] [--rounds 7] [--iters 3]

One process; per fill both paths are warmed up (every shape of the timed window), then padded and packed rounds ALTERNATE and
each round is timed with device events around ``iters`` forward + backward passes; median and min over the rounds are
reported per pass.  Train mode (dropout 0.1), random N(0, 0.02) weights, random token ids, seed fixed.  Length distribution:
fill 1.0 = every report T tokens; otherwise len_i ~ U{ceil(L/2) .. floor(3L/2)} with L = fill * T, clipped to [1, T], then the
first reports are nudged by +-1 until sum(len) = round(fill * n * T) exactly.  The attention masks live on the device, so a
packed call includes its one device-to-host read of the lengths.  Also reported: a graph-less forward (what the
micro-batched engine step re-runs) and torch.cuda.max_memory_allocated of one pass above the resident weights.
Prints one JSON object per fill and a final table; not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mammo_clip_amd  # noqa: E402,F401
from mammo_clip_amd.breastclip.model import clip as clipmod  # noqa: E402
from mammo_clip_amd.breastclip.model.modules import load_text_encoder  # noqa: E402


def lengths_for(fill, n, T, gen):
    if fill >= 1.0:
        return [T] * n
    L = fill * T
    lo, hi = max(1, -(-int(L) // 2)), min(T, int(1.5 * L))
    ln = torch.randint(lo, hi + 1, (n,), generator=gen).tolist()
    want, i = round(fill * n * T), 0
    while sum(ln) != want:
        step = 1 if sum(ln) < want else -1
        if 1 <= ln[i % n] + step <= T:
            ln[i % n] += step
        i += 1
    return ln


def tokens_for(ln, T, gen, dev):
    n = len(ln)
    ids = torch.randint(1000, 28996, (n, T), generator=gen)
    mask = (torch.arange(T)[None, :] < torch.tensor(ln)[:, None]).long()
    ids[:, 0] = 101
    ids[torch.arange(n), torch.tensor(ln) - 1] = 102
    ids = ids * mask
    return {"input_ids": ids.to(dev), "attention_mask": mask.to(dev), "token_type_ids": torch.zeros_like(ids).to(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=128, help="sequences per call (2b: both reports of b = 64 pairs)")
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--fills", default="1.0,0.5,0.25,0.1")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to measure on a CPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    te = load_text_encoder({"source": "huggingface", "name": "emilyalsentzer/Bio_ClinicalBERT", "pretrained": False,
                            "pooling": "eos"}, vocab_size=28996).to(dev).train()
    model = types.SimpleNamespace(text_encoder=te, text_pooling="eos")
    gen = torch.Generator().manual_seed(args.seed)
    r = torch.randn((args.seqs, 768), generator=gen).to(dev)

    def one_pass(tok, packed, backward=True):
        te.set_packed(packed)
        if backward:
            te.zero_grad(set_to_none=True)
            clipmod.BreastClip.encode_text(model, tok).backward(r)
        else:
            with torch.no_grad():
                clipmod.BreastClip.encode_text(model, tok)

    def timed(tok, packed, backward=True):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            one_pass(tok, packed, backward)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def peak(tok, packed):
        one_pass(tok, packed)
        te.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        one_pass(tok, packed)
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    rows = []
    for fill in [float(f) for f in args.fills.split(",")]:
        ln = lengths_for(fill, args.seqs, args.T, gen)
        tok = tokens_for(ln, args.T, gen, dev)
        for packed in (False, True):                       # warm-up: every shape of the timed window, both directions
            for _ in range(2):
                one_pass(tok, packed)
                one_pass(tok, packed, backward=False)
        torch.cuda.synchronize()
        t = {(p, bw): [] for p in (False, True) for bw in (True, False)}
        for _ in range(args.rounds):
            for packed in (False, True):
                t[(packed, True)].append(timed(tok, packed))
            for packed in (False, True):
                t[(packed, False)].append(timed(tok, packed, backward=False))
        row = {"fill": sum(ln) / (args.seqs * args.T), "seqs": args.seqs, "T": args.T, "tokens": sum(ln), "min_len": min(ln), "max_len": max(ln)}
        for p, name in ((False, "padded"), (True, "packed")):
            row[name + "_ms_median"], row[name + "_ms_min"] = statistics.median(t[(p, True)]), min(t[(p, True)])
            row[name + "_fwd_ms_median"], row[name + "_fwd_ms_min"] = statistics.median(t[(p, False)]), min(t[(p, False)])
            row[name + "_peak_mib"] = peak(tok, p)
        row["speedup_median"] = row["padded_ms_median"] / row["packed_ms_median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| fill | tokens | padded ms (median / min) | packed ms (median / min) | ratio | fwd only padded / packed ms | peak MiB padded / packed |")
    print("|---|---|---|---|---|---|---|")
    for w in rows:
        print(f"| {w['fill']:.2f} | {w['tokens']} | {w['padded_ms_median']:.2f} / {w['padded_ms_min']:.2f} | "
              f"{w['packed_ms_median']:.2f} / {w['packed_ms_min']:.2f} | {w['speedup_median']:.2f}x | "
              f"{w['padded_fwd_ms_median']:.2f} / {w['packed_fwd_ms_median']:.2f} | {w['padded_peak_mib']:.0f} / {w['packed_peak_mib']:.0f} |")


if __name__ == "__main__":
    main()
