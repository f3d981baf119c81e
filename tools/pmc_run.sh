#!/bin/bash
# Developer script: HBM traffic PMC passes (separate runs, kernel-trace only)
# of bench.py --full, run from the repository root; output under $1 (default
# pmc_out), summary -> $1/pmc_traffic.json
set -e
O=${1:-pmc_out}
mkdir -p $O
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 300 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $O/bench_$C -o run -- python3 bench.py --full --steps 3 --warmup 1 --settle-s 0 --no-cpu-baseline > $O/bench_$C.log 2>&1
done
python3 tools/pmc_traffic.py $O/bench_FETCH_SIZE $O/bench_WRITE_SIZE $O/pmc_traffic.json
echo done
