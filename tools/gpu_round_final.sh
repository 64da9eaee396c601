# End-of-round measurements against one kernel build, in GPU calls of a few
# minutes each (STAGE):
#   profile  rocprofv3 kernel trace + PMC passes per config (PCFGS), folded
#            into profiles/pmc_<cfg>.json and profiles/$ROUND/kernel_stats_*
#            (tools/gpu_profile_round.sh);
#   bench    the default bench line with everything in it (--full), then
#            every config's own line (tools/gpu_bench_all.sh; SKIP_PYTEST=1
#            to leave the GPU tests out) -- after `profile`, so every line
#            joins the counters of its own build.
# Outputs under $OUT (default bench_out/); copy what is kept into
# profiles/$ROUND/.
set -u
export OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
export ROUND=${ROUND:-round5}
case ${STAGE:-bench} in
profile)
  bash tools/gpu_profile_round.sh ;;
bench)
  timeout -k 10 600 python bench.py --full > $OUT/bench_default.log 2>&1
  rc=$?; echo "bench default rc=$rc"; tail -1 $OUT/bench_default.log | cut -c1-300
  [ $rc -ne 0 ] && exit $rc
  bash tools/gpu_bench_all.sh ;;
trace_default)
  # the whole default line (--full) under the kernel tracer: its dominant
  # kernels' trace averages against the line's HIP-event kernel times
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_default -o run --output-format csv -- python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_default_traced.log 2>&1
  rc=$?; echo "trace default rc=$rc"; [ $rc -ne 0 ] && exit $rc
  python3 tools/default_trace_summary.py $OUT/prof_default/run_kernel_stats.csv $OUT/bench_default_traced.log $OUT/prof_default/run_kernel_trace.csv > $OUT/default_cmd_trace_summary.json &&
  cp $OUT/prof_default/run_kernel_stats.csv $OUT/kernel_stats_default_cmd.csv &&
  rm -f $OUT/prof_default/run_kernel_trace.csv && cat $OUT/default_cmd_trace_summary.json ;;
*)
  echo "STAGE=profile|bench|trace_default" >&2; exit 2 ;;
esac
