#!/usr/bin/env python3
"""Instruction mix of the lane = column depthwise kernels from the ISA (developer tool).

Per instantiation <K,S,NCOL,MODE,G,KC> of lane::dwconv_lane_fwd_kernel it reports ONE steady-state phase of the software
pipeline -- the code between two s_barrier that holds a block's stencil FMAs; of the U unrolled phases the shortest one --
as every wave executes it:
  * the descriptor refill (wave 0 only, once per 64 blocks: the branch-guarded region with the integer divisions) and
    whatever precedes the loop header in the first phase's text are EXCLUDED (their sizes are printed beside it);
  * executed VALU instructions by category:
      stencil    packed FMAs / MULs of the stencil itself -- by construction RB rows x matching tap rows x K x NCOL, twice
                 that where the weight gradient rides along (MODE 3 / 5); counted by that formula, capped by what is there
      pk_f32     every other packed f32 instruction (BatchNorm FMAs, SiLU products, statistics)
      f32        single f32 arithmetic
      trans      transcendentals (v_exp_f32 / v_rcp_f32 / ...), listed as exp+rcp
      unpack     16 bit -> f32 (shift by 16 / mask 0xffff0000 / v_cvt_f32_f16)
      pack       f32 -> 16 bit (v_cvt_pk_*)
      cmp/sel    v_cmp* / v_cndmask*
      int        the remaining integer / address / bit instructions
      mov        v_mov* / v_accvgpr*
      lane       v_readlane / v_writelane / v_readfirstlane / v_mbcnt / DPP forms
    MFMA instructions are listed apart (they issue to the matrix core);
  * issue-weighted VALU cycles: 8 per transcendental, 4 per other VALU instruction;
  * conditional branches after the first stencil FMA of the phase (a straight-line block body has none), s_nop, s_waitcnt;
  * VGPRs, spilled VGPRs / SGPRs and scratch bytes of the kernel (code-object metadata), v_readlane_b32 of the whole body.

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -S --cuda-device-only mammo_clip_amd/csrc/conv_lane.hip -o conv_lane.s
       python scripts/lane_isa_mix.py conv_lane.s
       python scripts/lane_isa_mix.py --compare old.s new.s"""
import collections
import re
import sys

KERNEL = re.compile(r"^(_ZN4lane22dwconv_lane_fwd_kernelI(\w+?)EEv\w+):[^\n]*\n(.*?)s_endpgm", re.S | re.M)
PACKED = ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32")
TRANS = ("v_exp_f32", "v_rcp_f32", "v_rcp_iflag_f32", "v_log_f32", "v_sqrt_f32", "v_rsq_f32", "v_sin_f32", "v_cos_f32")
CATS = ("stencil", "pk_f32", "f32", "trans", "unpack", "pack", "cmp/sel", "int", "mov", "lane")
RB = 4


def base(op):
    return re.sub(r"_(e32|e64|sdwa|dpp|e64_dpp)$", "", op)


def category(op, text):
    b = base(op)
    if op.endswith("dpp") or b in ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32", "v_mbcnt_lo_u32_b32", "v_mbcnt_hi_u32_b32"):
        return "lane"
    if b in PACKED:
        return "pk_f32"
    if b in TRANS:
        return "trans"
    if b.startswith("v_mfma") or b.startswith("v_smfma"):
        return "mfma"
    if b.startswith("v_cvt_pk") or b in ("v_cvt_f16_f32", "v_pack_b32_f16"):
        return "pack"
    if b == "v_cvt_f32_f16" or re.match(r"v_lshlrev_b32\w* v\d+, 16, ", text) or re.match(r"v_and_b32\w* v\d+, 0xffff0000, ", text):
        return "unpack"
    if b.startswith("v_cmp") or b.startswith("v_cndmask"):
        return "cmp/sel"
    if b.startswith("v_mov") or b.startswith("v_accvgpr"):
        return "mov"
    if re.match(r"v_(add|sub|mul|fma|fmac|fmamk|fmaak|mac|mad|max|min|trunc|floor|rndne|ldexp)\w*_f32$", b):
        return "f32"
    return "int"


def stencil_by_formula(K, S, NCOL, MODE):
    """packed FMAs / MULs a phase's stencil needs: RB input rows, the tap rows kh with (row - kh) % S == 0, K x NCOL each (the same
    in every phase: the rotation period is even where S == 2)"""
    rows = sum(1 for j in range(RB) for kh in range(K) if (j - kh) % S == 0)
    return rows * K * NCOL * (2 if MODE in (3, 5) else 1)


def items_of(body):
    """[(is_label, opcode or label, text)] of a kernel body"""
    out = []
    for ln in body.splitlines():
        t = ln.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":"):
            out.append((True, t[:-1], t))
        elif not t.startswith("."):
            out.append((False, t.split()[0], t))
    return out


def branch_target(text):
    m = re.match(r"s_c?branch\w*\s+(\S+)", text)
    return m.group(1) if m else None


def has_tap(text):
    """a packed instruction with an SGPR PAIR as a source, both halves used (a tap of the wave's channel pair) -- not a scalar
    constant broadcast to both halves (op_sel_hi 0 at that source)"""
    srcs = re.split(r",\s*", re.sub(r"\s+op_sel.*$", "", text.split(None, 1)[1]))[1:]
    hi = re.search(r"op_sel_hi:\[([\d,]+)\]", text)
    hi = [int(v) for v in hi.group(1).split(",")] if hi else [1] * len(srcs)
    return any(o.startswith("s[") and hi[k] == 1 for k, o in enumerate(srcs))


def analyse(name, body, meta):
    K, S, NCOL, MODE = (int(v) for v in name.split(",")[:4])
    its = items_of(body)
    label_at = {op: i for i, (lab, op, _) in enumerate(its) if lab}
    # pipeline intervals: the text between two s_barrier
    bounds = [-1] + [i for i, (lab, op, _) in enumerate(its) if not lab and op == "s_barrier"]
    phases = []
    for lo, hi in zip(bounds, bounds[1:]):
        lo += 1
        if sum(1 for lab, op, _ in its[lo:hi] if not lab and base(op) in ("v_pk_fma_f32", "v_pk_mul_f32")) < 16:
            continue
        # the first phase's text starts before the loop: cut at the loop header = the first label that a branch BEHIND the
        # interval jumps back to
        pre = 0
        for i in range(lo, hi if not phases else lo):
            if its[i][0] and any(not lab and branch_target(t) == its[i][1] for lab, _, t in its[hi:]):
                pre = sum(1 for lab, _, _ in its[lo:i] if not lab)
                lo = i
                break
        # the refill: forward-branch-guarded regions with an integer division and no packed f32, exponential or global access
        drop = set()
        for i in range(lo, hi):
            if its[i][0]:
                continue
            tgt = branch_target(its[i][2])
            j = label_at.get(tgt, -1)
            if i < j <= hi:
                ops = [base(op) for lab, op, _ in its[i + 1:j] if not lab]
                if "v_rcp_iflag_f32" in ops and not any(o in PACKED or o == "v_exp_f32" or o.startswith("global_") for o in ops):
                    drop.update(range(i + 1, j))
        kept = [(op, t) for i, (lab, op, t) in enumerate(its[lo:hi], lo) if not lab and i not in drop]
        refill = sum(1 for i in drop if not its[i][0])
        phases.append((kept, refill, pre))
    if not phases:
        return None
    kept, _, _ = min(phases, key=lambda p: len(p[0]))
    r = collections.OrderedDict()
    r["name"], r["phases"] = name, len(phases)
    r["refill"] = "+".join(str(p[1]) for p in phases)
    r["pre"] = max(p[2] for p in phases)
    r["instr"] = len(kept)
    cats = collections.Counter()
    for op, t in kept:
        if op.startswith("v_"):
            cats[category(op, t)] += 1
    st = min(stencil_by_formula(K, S, NCOL, MODE), cats["pk_f32"])
    cats["stencil"], cats["pk_f32"] = st, cats["pk_f32"] - st
    r["cats"] = cats
    r["valu"] = sum(cats[c] for c in CATS)
    r["mfma"] = cats["mfma"]
    r["cycles"] = 4 * r["valu"] + 4 * cats["trans"]
    r["exp"] = sum(1 for op, _ in kept if base(op) == "v_exp_f32")
    r["rcp"] = sum(1 for op, _ in kept if base(op) == "v_rcp_f32")
    # first stencil FMA: the first packed FMA / MUL with a tap (an SGPR pair) as an operand; the weight-gradient mode has its
    # taps' accumulators in VGPRs: there, the first packed FMA behind the last global load
    first = next((i for i, (op, t) in enumerate(kept) if base(op) in ("v_pk_fma_f32", "v_pk_mul_f32") and has_tap(t)), None)
    if first is None or MODE == 2:
        last_ld = max([i for i, (op, _) in enumerate(kept) if op.startswith("global_load")] + [0])
        first = next((i for i, (op, _) in enumerate(kept) if i > last_ld and base(op) in ("v_pk_fma_f32", "v_pk_mul_f32")), len(kept))
    r["cbr"] = sum(1 for op, _ in kept[first:] if op.startswith("s_cbranch"))
    r["cbr_all"] = sum(1 for op, _ in kept if op.startswith("s_cbranch"))
    r["nop"] = sum(1 for op, _ in kept if op == "s_nop")
    r["wait"] = sum(1 for op, _ in kept if op == "s_waitcnt")
    r["lds"] = sum(1 for op, _ in kept if op.startswith("ds_"))
    r["salu"] = sum(1 for op, _ in kept if op.startswith("s_"))
    r["readlane"] = sum(1 for lab, op, _ in its if not lab and op == "v_readlane_b32")
    r.update(meta)
    return r


def metadata(src):
    out = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", src, re.S):
        f = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|sgpr_spill_count|vgpr_count|vgpr_spill_count):\s+(\d+)", m.group(2))}
        out[m.group(1)] = {"vgpr": f.get("vgpr_count", -1), "vspill": f.get("vgpr_spill_count", -1),
                           "sspill": f.get("sgpr_spill_count", -1), "scratch": f.get("private_segment_fixed_size", -1)}
    return out


def table(path):
    src = open(path).read()
    meta = metadata(src)
    rows = collections.OrderedDict()
    for m in KERNEL.finditer(src):
        name = m.group(2).replace("Li", "").replace("E", ",").rstrip(",")
        r = analyse(name, m.group(3), meta.get(m.group(1), {"vgpr": -1, "vspill": -1, "sspill": -1, "scratch": -1}))
        if r:
            rows[name] = r
    return rows


def print_table(rows):
    print("# steady-state phase (shortest of the unrolled phases; descriptor refill and pre-loop text excluded)")
    print(f"{'K,S,NCOL,MODE,G,KC':19s} {'instr':>5s} {'VALU':>5s} {'cyc':>5s} | " + " ".join(f"{c:>7s}" for c in CATS) +
          f" | {'exp+rcp':>7s} {'mfma':>4s} {'LDS':>4s} {'SALU':>4s} | {'cbr':>3s} {'cbr*':>4s} {'nop':>4s} {'wait':>4s} | {'VGPR':>4s} {'vspl':>4s} {'sspl':>4s} {'scr B':>5s} {'rdlane':>6s} | {'phases':>6s} {'refill (excluded)':>17s} {'pre':>4s}")
    for r in rows.values():
        c = r["cats"]
        print(f"{r['name']:19s} {r['instr']:5d} {r['valu']:5d} {r['cycles']:5d} | " + " ".join(f"{c[k]:7d}" for k in CATS) +
              f" | {r['exp']:3d}+{r['rcp']:<3d} {r['mfma']:4d} {r['lds']:4d} {r['salu']:4d} | {r['cbr']:3d} {r['cbr_all']:4d} {r['nop']:4d} {r['wait']:4d} | "
              f"{r['vgpr']:4d} {r['vspill']:4d} {r['sspill']:4d} {r['scratch']:5d} {r['readlane']:6d} | {r['phases']:6d} {r['refill']:>17s} {r['pre']:4d}")
    print("# cyc = 4 x VALU + 4 x trans (issue-weighted: a transcendental costs 8); cbr = conditional branches after the first stencil FMA of the")
    print("# phase, cbr* = in the whole phase; rdlane = v_readlane_b32 in the whole kernel body; refill = instructions of the excluded refill")
    print("# region per phase; pre = pre-loop instructions cut from the first phase's text")


def print_compare(old, new):
    print("# old -> new per instantiation: instr / VALU / issue-weighted cycles / exp+rcp / cond. branches after the first stencil FMA / s_nop / VGPRs / scratch bytes")
    for name, n in new.items():
        o = old.get(name)
        if o is None:
            print(f"{name:19s} (new)")
            continue
        f = lambda r: f"{r['instr']:4d} / {r['valu']:4d} / {r['cycles']:4d} / {r['exp']:2d}+{r['rcp']:<2d} / {r['cbr']:2d} / {r['nop']:3d} / {r['vgpr']:3d} / {r['scratch']:3d}"
        flag = ""
        if n["scratch"] > o["scratch"] or n["vspill"] > o["vspill"]:
            flag += "  MORE SPILL"
        if n["cycles"] > o["cycles"]:
            flag += "  more cycles"
        print(f"{name:19s} {f(o)}  ->  {f(n)}   cyc {100.0 * (n['cycles'] - o['cycles']) / o['cycles']:+5.1f} %{flag}")
    for name in old:
        if name not in new:
            print(f"{name:19s} (gone)")


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--compare":
        print_compare(table(a[1]), table(a[2]))
    else:
        print_table(table(a[0] if a else "conv_lane.s"))
