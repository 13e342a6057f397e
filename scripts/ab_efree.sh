#!/bin/bash
# A/B of the E-free stride-1 3x3 blocks (MC_EFREE: fused forward + fused backward with e rows from the block input) on one box
O=${OUT:-bench_out}; mkdir -p $O
run() { local name=$1; shift; local envs=(); while [ "$1" != "--" ]; do envs+=("$1"); shift; done; shift
  env "${envs[@]}" python bench.py --full --no-cpu-baseline --no-n8-load --no-parity --roofline-in-timed-region "$@" 2>$O/abe_$name.err | tail -1 > $O/abe_$name.json
  python - "$name" "$O" <<'PY'
import json, sys
n, o = sys.argv[1], sys.argv[2]
try:
    r = json.load(open(f"{o}/abe_{n}.json"))
    print(f"{n:24s} {r['value']:9.2f} pairs/s {r['ms_per_step']:10.1f} ms  peak {r['config']['peak_hbm_gb']} GB  loss {r['config']['loss']}  tagged GB/step {r['whole_step']['algorithmic_gb_per_step']}")
except Exception as e:
    print(n, "FAILED", e)
PY
}
run cfg3_e0 MC_EFREE=0 -- --workload cfg3 --steps 8 --warmup 2
run cfg3_e1 MC_EFREE=1 -- --workload cfg3 --steps 8 --warmup 2
run cfg2_e0 MC_EFREE=0 -- --workload cfg2 --steps 8 --warmup 2
run cfg2_e1 MC_EFREE=1 -- --workload cfg2 --steps 8 --warmup 2
run cfg4_e0 MC_EFREE=0 -- --steps 2 --warmup 1
run cfg4_e1 MC_EFREE=1 -- --steps 2 --warmup 1
run n8_e0 MC_EFREE=0 -- --as-gpus 8 --steps 3 --warmup 1
run n8_e1 MC_EFREE=1 -- --as-gpus 8 --steps 3 --warmup 1
