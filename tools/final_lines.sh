#!/bin/bash
# every bench line README / DESIGN quote, one box, one after the other -> gpurun_out/final_lines.jsonl (committed as profiles/rNN_bench_lines.jsonl)
set -u
mkdir -p gpurun_out; export TMPDIR=/tmp
out=gpurun_out/final_lines.jsonl; : > $out
run() { # args of bench.py
  timeout -k 10 400 python3 bench.py "$@" > gpurun_out/final_one.log 2>&1
  rc=$?
  grep -h '^{"metric"' gpurun_out/final_one.log >> $out
  echo "bench.py $* -> rc=$rc ($(grep -c . $out) lines)"
  [ $rc -ge 124 ] && exit $rc
  return 0
}
run --full
run --full --workload c2
run --full --workload c3
run --full --workload fe
run --full --workload fe_bcsr
run --full --workload fe_spmm4
run --full --workload fe_spmm8
run --full --workload mesh
run --full --workload c2_perm
run --full --workload c2_perm --internal
run --full --workload fe_perm
run --full --workload mesh_perm --internal
run --full --cold --steps 30 --warmup 3 --no-cpu-baseline
echo FINAL_DONE
