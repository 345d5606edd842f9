# usage (on the GPU box, from the repo root):  bash tools/profile_round.sh r02
# Produces under $OUT (default out/): <R>_kernel_stats.csv (rocprofv3 --kernel-trace --stats of the default bench command),
# <R>_bench_under_rocprof.json, <R>_pmc_hbm_traffic_per_launch.json (FETCH_SIZE / WRITE_SIZE, separate passes),
# <R>_mfma_busy.json (SQ instruction / busy counters per kernel).  Copy what is to be judged into profiles/.
# The program sits directly after `--` (no env / bash -c hop: the profiler's preloaded library has initialised the GPU).
set -e
R=${1:-r02}
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}
mkdir -p $OUT
# Per-kernel durations are only comparable with bench.py's `roofline` (measured in its single-stream region) when nothing co-runs: the stats and
# counter passes run the whole command on ONE stream (exported, not `env`: the program must sit directly after `--`); a second stats pass
# records the product schedule (teacher pass and weight gradients on side streams) for the co-running picture.
export PFST_WGRAD_STREAM=0 PFST_FORK_TEACHER=0
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_stats -o s -- python3 bench.py --full --no-alt-math > $OUT/${R}_bench_under_rocprof.json 2> $OUT/b_under_rocprof.err
echo stats done
unset PFST_WGRAD_STREAM PFST_FORK_TEACHER
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_stats_ov -o s -- python3 bench.py --full --no-alt-math --no-cpu-baseline > $OUT/${R}_bench_under_rocprof_overlap.json 2> $OUT/b_under_rocprof_ov.err
find $OUT/prof_stats_ov -name "*kernel_stats.csv" -exec cp {} $OUT/${R}_kernel_stats_overlap.csv \;
rm -rf $OUT/prof_stats_ov
echo overlap stats done
export PFST_WGRAD_STREAM=0 PFST_FORK_TEACHER=0
ARGS="--steps 1 --warmup 1 --no-cpu-baseline --no-alt-math --no-kernel-timing"
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o f -- python3 bench.py $ARGS > $OUT/pmc_f.log 2>&1
echo fetch done
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o w -- python3 bench.py $ARGS > $OUT/pmc_w.log 2>&1
echo write done
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_sq -o q -- python3 bench.py $ARGS > $OUT/pmc_q.log 2>&1
echo sq done
python3 tools/pmc_summary.py $OUT/pmc_fetch $OUT/pmc_write $OUT/${R}_pmc_hbm_traffic_per_launch_${MATH:-f16x3}.json > /dev/null
python3 tools/pmc_mfma.py $OUT/pmc_sq $OUT/${R}_mfma_busy.json > /dev/null
find $OUT/prof_stats -name "*kernel_stats.csv" -exec cp {} $OUT/${R}_kernel_stats.csv \;
rm -rf $OUT/prof_stats $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_sq
ls -la $OUT | tail -8
