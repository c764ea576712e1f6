# Bench lines for the other BASELINE configs on one GPU (config 4, config 5, config 3's per-GPU share).
set -o pipefail
cd $GRAFT_REPO_ROOT
# the full bench lines (CPU baseline, parity, roofline) go to $BENCH_OUT (default: bench_out/)
O=${BENCH_OUT:-bench_out}; mkdir -p $O
timeout -k 10 400 python bench.py --full --config config4 --steps 5 --warmup 2 > $O/bench_config4.log 2> $O/bench_config4.err || { tail -20 $O/bench_config4.err; exit 1; }
tail -1 $O/bench_config4.log | cut -c1-300
timeout -k 10 300 python bench.py --full --config config5 --steps 10 --warmup 3 > $O/bench_config5.log 2> $O/bench_config5.err || { tail -20 $O/bench_config5.err; exit 1; }
tail -1 $O/bench_config5.log | cut -c1-300
timeout -k 10 300 python bench.py --pop 128 --steps 10 --warmup 3 --no-cpu-baseline > gpurun_out/bench_pop128.log 2> gpurun_out/bench_pop128.err || { tail -20 gpurun_out/bench_pop128.err; exit 1; }
tail -1 gpurun_out/bench_pop128.log | cut -c1-300
