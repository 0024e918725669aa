#!/bin/bash
# Vectored-encode bench lines (bench.py --full --iov) for c1 / c3 / c0.
# Logs go to $OUT (defaults to ./bench_out).
set -u
OUT=${OUT:-$PWD/bench_out}
mkdir -p $OUT
for wl in ${WLS:-c1 c3 c0}; do
  timeout -k 10 300 python bench.py --full --workload $wl --iov --no-cpu-baseline --c4-leg off ${BARGS:-} > $OUT/iov_$wl.log 2>&1
  rc=$?; echo "iov $wl rc=$rc"
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);r=d['roofline'];print(sys.argv[1].split('/')[-1], round(d['value'],1), round(d['ms_per_step']*1e3,1), 'valid', d['validated'], r['kernel'], round(r['avg_launch_us'],1), 'frac', round(r['frac'],3), 'step_frac', round(r['step_frac'],3), {k.replace('_kernel',''):round(v['avg_us'],1) for k,v in d['kernels_breakdown_pass'].items()})" $OUT/iov_$wl.log
  [ $rc -eq 0 ] || exit $rc
done
