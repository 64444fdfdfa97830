cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-results}
mkdir -p $OUT
rocprofv3 --kernel-trace --stats -d $OUT/prof_r1e_full -o out --output-format csv -- python bench.py --full --no-cpu > $OUT/r01e_bench_full_profiled_stdout.json 2> $OUT/r01e_prof_full.log || exit 1
head -12 $OUT/prof_r1e_full/out_kernel_stats.csv | cut -c1-150
