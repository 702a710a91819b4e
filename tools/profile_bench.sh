#!/bin/bash
# Round artefacts: the --full bench line + its detail file, and rocprofv3 kernel stats of the same command (shortened), written to $OUT (default bench_out/) for profiles/.
# usage on the GPU box: bash tools/profile_bench.sh <tag>
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}; mkdir -p $OUT
TAG=${1:-rXX}
cd $R && python bench.py --full > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err
tail -c 600 $OUT/${TAG}_bench_default.err
cp $R/bench_out/bench_detail_n1.json $OUT/${TAG}_bench_detail_n1.json   # (the shortened run below rewrites the detail file)
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_bench
BEVGEN_BENCH_NO_PMC=1 rocprofv3 --kernel-trace --stats -d $OUT/prof_bench -o bench -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-extra-legs --no-decode-leg --no-exact-leg > $OUT/${TAG}_bench_under_rocprof.json 2> $OUT/prof_bench.err
DB=$(find $OUT/prof_bench -name "*.db" | head -1)
python $R/tools/rocpd_kernel_stats.py $DB > $OUT/${TAG}_bench_kernel_stats.csv
rm -rf $OUT/prof_bench
head -c 1500 $OUT/${TAG}_bench_default.json; echo; head -12 $OUT/${TAG}_bench_kernel_stats.csv | cut -c1-160
