cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-results}
mkdir -p $OUT
python bench.py --full > $OUT/r01e_bench_stdout.json 2> $OUT/r01e_bench_stderr.log || exit 1
tail -c 600 $OUT/r01e_bench_stdout.json
rocprofv3 --kernel-trace --stats -d $OUT/prof_r1e -o out --output-format csv -- python bench.py --no-extra > $OUT/r01e_bench_profiled_stdout.json 2> $OUT/r01e_prof.log || exit 1
head -5 $OUT/prof_r1e/out_kernel_stats.csv | cut -c1-200
