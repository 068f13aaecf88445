# round-2 profile: kernel stats of the DEFAULT bench command, HBM traffic counters, in-kernel phase stamps
set -e
cd $GRAFT_REPO_ROOT
export OUT=${OUT:?set OUT to the folder the outputs go to}
export TMPDIR=/tmp
TAG=${1:-r02a}
mkdir -p $OUT/prof_$TAG $OUT/pmc_fetch_$TAG $OUT/pmc_write_$TAG
rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python bench.py --full > $OUT/prof_$TAG/bench_line.json 2> $OUT/prof_$TAG/err.txt
tail -c 1500 $OUT/prof_$TAG/bench_line.json
rm -f $OUT/prof_$TAG/run_kernel_trace.csv $OUT/prof_$TAG/*/run_kernel_trace.csv
echo stats done
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_fetch_$TAG -o run --output-format csv -- python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-sequential > $OUT/pmc_fetch_$TAG/log.txt 2>&1
echo fetch done
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_write_$TAG -o run --output-format csv -- python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-sequential > $OUT/pmc_write_$TAG/log.txt 2>&1
echo write done
rm -f $OUT/pmc_*_$TAG/run_kernel_trace.csv $OUT/pmc_*_$TAG/*/run_kernel_trace.csv
python scratch/stamps.py > $OUT/stamps_$TAG.txt 2>&1 || true
cat $OUT/stamps_$TAG.txt | tail -4
du -sh $OUT/prof_$TAG $OUT/pmc_fetch_$TAG $OUT/pmc_write_$TAG
