O=${OUT:-bench_out}/r04; mkdir -p $O
timeout 900 python -m pytest tests -m gpu -q > $O/pytest_gpu.txt 2>&1; tail -2 $O/pytest_gpu.txt
for wl in cfg1 cfg2 cfg3; do python bench.py --full --workload $wl --steps 10 --warmup 3 --no-cpu-baseline 2>/dev/null | tail -1 > $O/bench_$wl.json; done
python bench.py --full 2>/dev/null | tail -1 > $O/bench_cfg4.json
python bench.py --full --workload cfg5 --no-cpu-baseline 2>/dev/null | tail -1 > $O/bench_cfg5.json
for n in 2 4; do python bench.py --full --as-gpus $n --no-cpu-baseline 2>/dev/null | tail -1 > $O/bench_as$n.json; done
for f in $O/bench_*.json; do python -c "import json,sys; d=json.loads(open('$f').read()); print('$f', d['value'], d['ms_per_step'], d['config'].get('peak_reserved_gb'))"; done
