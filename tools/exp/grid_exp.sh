set -e
O=${1:-grid_exp_out}
mkdir -p $O
for M in 1 2 4 1000; do
  UPLINK_EXP_GRID_MULT=$M timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-other-configs --steps 5 > $O/bench_m$M.log 2>&1
done
echo done
