# Round-2 rocprofv3 evidence (run on the GPU box through gpurun); everything lands in gpurun_out/prof_r2/.
#   1. kernel trace + stats of the default bench command (cfg4, 1 step = 32 micro-batches)      -> cfg4_kernel_stats.csv
#   2. kernel trace + stats of one cfg3 step (32 pairs in one pass)                              -> cfg3_kernel_stats.csv
#   3. PMC passes over one cfg3 step, ALL kernels, one counter group per pass (FETCH_SIZE / WRITE_SIZE /
#      SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE + SQ_BUSY_CU_CYCLES)                           -> cfg3_pmc_<group>.csv (per kernel)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=/root/repo
OUT=$R/gpurun_out/prof_r2; mkdir -p $OUT
C4="python $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline"
C3="python $R/bench.py --full --workload cfg3 --steps 1 --warmup 1 --no-cpu-baseline"
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_c4 -- $C4 > $OUT/c4.log 2>&1
cp $(ls /tmp/p_c4/*/*kernel_stats.csv | head -1) $OUT/cfg4_kernel_stats.csv
cp $(ls /tmp/p_c4/*/*agent_info.csv | head -1) $OUT/agent_info.csv
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_c3 -- $C3 > $OUT/c3.log 2>&1
cp $(ls /tmp/p_c3/*/*kernel_stats.csv | head -1) $OUT/cfg3_kernel_stats.csv
i=0
for grp in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CU_CYCLES"; do
  i=$((i+1))
  timeout 900 rocprofv3 --kernel-trace --pmc $grp --output-format csv -d /tmp/p_pmc$i -- $C3 > $OUT/pmc$i.log 2>&1
  f=$(ls /tmp/p_pmc$i/*/*counter_collection.csv 2>/dev/null | head -1)
  [ -z "$f" ] && { echo "pass $i produced no counters"; tail -3 $OUT/pmc$i.log; continue; }
  python - "$f" "$OUT/cfg3_pmc_$(echo $grp | cut -d' ' -f1).csv" <<'PY'
import csv, sys, collections
agg = collections.OrderedDict()
for r in csv.DictReader(open(sys.argv[1])):
    k = (r['Kernel_Name'], r['Counter_Name'])
    a = agg.setdefault(k, [0, 0.0])
    a[0] += 1; a[1] += float(r['Counter_Value'])
with open(sys.argv[2], 'w') as f:
    w = csv.writer(f); w.writerow(['kernel', 'counter', 'launches', 'sum', 'avg'])
    for (k, c), (n, s) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        w.writerow([k, c, n, s, s / n])
PY
done
ls -la $OUT
