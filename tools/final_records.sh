set -o pipefail
export OUT=${OUT:-out}          # output directory (also for tools/profile_round.sh)
mkdir -p $OUT
python -m pytest tests -m gpu -x -q > $OUT/r05_gpu_tests.log 2>&1; echo suite rc=$?; tail -2 $OUT/r05_gpu_tests.log
python bench.py --steps 20 --warmup 5 --full > $OUT/r05_bench_20steps.json 2> $OUT/r05_bench.err && echo bench done
bash tools/profile_round.sh r05 > $OUT/r05_profile_round.log 2>&1; echo profile rc=$?
PFST_WGRAD_STREAM=0 PFST_FORK_TEACHER=0 python bench.py --steps 4 --warmup 2 --full --per-layer --no-cpu-baseline --no-alt-math > $OUT/r05_per_layer.json 2> $OUT/r05_per_layer_f16x3.txt; echo per-layer rc=$?
