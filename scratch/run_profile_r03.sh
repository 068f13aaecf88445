# round-3 evidence, ONE rocprofv3 pass per gpurun call (two passes in one call stalled between them once):
#   OUT=<folder> bash scratch/run_profile_r03.sh stats|fetch|write [TAG]     then, where summarize_r03.py finds the passes:  python scratch/summarize_r03.py TAG
set -e
cd $GRAFT_REPO_ROOT
export OUT=${OUT:?set OUT to the folder the outputs go to}
export TMPDIR=/tmp
export GCN_MAXCUT_BENCH_SERIAL_GEN=1   # no forked graph-generation workers under the profiler (they hang now and then once its library has initialised the GPU)
PASS=${1:-stats}
TAG=${2:-r03a}
SMALL="--steps 5 --warmup 1 --no-cpu-baseline --no-sequential --no-other-workloads --no-dp-profile"
case $PASS in
  stats) mkdir -p $OUT/prof_$TAG
         rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python bench.py --full > $OUT/prof_$TAG/bench_line.json 2> $OUT/prof_$TAG/err.txt ;;
  fetch) mkdir -p $OUT/pmc_fetch_$TAG
         rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_fetch_$TAG -o run --output-format csv -- python bench.py --full $SMALL > $OUT/pmc_fetch_$TAG/log.txt 2>&1 ;;
  write) mkdir -p $OUT/pmc_write_$TAG
         rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_write_$TAG -o run --output-format csv -- python bench.py --full $SMALL > $OUT/pmc_write_$TAG/log.txt 2>&1 ;;
esac
echo $PASS done
