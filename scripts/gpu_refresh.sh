#!/bin/bash
# refresh of the judged evidence on the GPU box: bench lines of every workload + rocprofv3 stats / PMC of the default one
# usage: scripts/gpu_refresh.sh <tag> <out dir>   -> <out dir>/<tag>/bench_*.json; the profiles where scripts/profile_gpu.sh puts them
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
TAG=$1
OUT=$2/$TAG
cd $ROOT
mkdir -p $OUT
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
for w in real c48l80 config1; do
  python bench.py --full --workload $w --cpu_rotations 0 > $OUT/bench_$w.json 2> $OUT/bench_$w.err
done
bash scripts/profile_gpu.sh $TAG > $OUT/profile.log 2>&1
tail -30 $OUT/profile.log
