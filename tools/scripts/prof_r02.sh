# Round-2 final evidence: full bench line, the same command under rocprofv3 --kernel-trace --stats, a whole bench run with extras
# under the profiler, the e2e decode step per kernel.  Usage (gpurun): bash tools/scripts/prof_r02.sh <tag>
tag=${1:-r02z}
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-results}
mkdir -p $OUT
python bench.py --full > $OUT/${tag}_bench_full.json 2> $OUT/${tag}_bench_full.err || exit 1
echo "bench done"
rocprofv3 --kernel-trace --stats -d $OUT/${tag}_prof -o out --output-format csv -- python3 bench.py --no-extra --no-cpu > $OUT/${tag}_bench_profiled_stdout.json 2> $OUT/${tag}_prof.log || exit 1
python tools/summarize_kernel_trace.py $OUT/${tag}_prof 12 --last 200 gemm_tile_kernel > $OUT/${tag}_bench_kernel_trace_summary.txt 2>&1
find $OUT/${tag}_prof -name '*kernel_stats.csv' -exec cp {} $OUT/${tag}_bench_kernel_stats.csv \;
rm -rf $OUT/${tag}_prof
echo "profiled bench done"
for att in cache current; do
  rocprofv3 --kernel-trace --stats -d $OUT/${tag}_prof_e2e_$att -o out --output-format csv -- python3 tools/e2e_profile.py 28 $att > $OUT/${tag}_e2e_$att.json 2> $OUT/${tag}_e2e_$att.log || exit 1
  python tools/summarize_kernel_trace.py $OUT/${tag}_prof_e2e_$att 30 > $OUT/${tag}_e2e_${att}_kernel_summary.txt 2>&1
  rm -rf $OUT/${tag}_prof_e2e_$att
done
echo "e2e profiles done"
