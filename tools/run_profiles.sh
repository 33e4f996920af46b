#!/bin/bash
# Round profiles on the GPU box (from the repo root):  bash tools/run_profiles.sh TAG CONFIG OUT
#   kernel trace + stats, then one rocprofv3 --pmc pass per counter (the guide's rule: counters in their own runs).
# Results land under OUT/prof_${TAG}_*; condense them here with tools/prof_summary.py.
set -o pipefail
TAG=$1; CFG=${2:-C2}; OUT=${3:?usage: bash tools/run_profiles.sh TAG CONFIG OUT}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
ARGS="bench.py --config $CFG --no-cpu-baseline --no-extras --steps 12 --warmup 3"
export CESX_BENCH_PREWARM_S=${CESX_BENCH_PREWARM_S:-0.3}
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_k -- python3 $ARGS > $OUT/prof_${TAG}_k.log 2>&1 || exit 2
# (--pmc serialises the streams' kernels: a kernel of the caller's stream that polls for one of the side stream would wait
#  for its time-out -- the engine recovers, bench.py carries on, but the event join is the honest mode for these passes)
export CESX_POLL_JOIN=0
for ctr in FETCH_SIZE WRITE_SIZE SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE; do
  rocprofv3 --pmc $ctr --output-format csv -d $OUT/prof_${TAG}_$ctr -- python3 $ARGS > $OUT/prof_${TAG}_$ctr.log 2>&1 || exit 3
done
unset CESX_POLL_JOIN
# condense on the box (the raw counter CSVs are large): the summaries land in profiles/ of the box's copy of the tree and
# are copied to OUT/prof_out/; the raw directories are removed
python3 tools/prof_summary.py ${TAG}:${CFG} $OUT/prof_${TAG}_k $OUT/prof_${TAG}_FETCH_SIZE $OUT/prof_${TAG}_WRITE_SIZE \
    $OUT/prof_${TAG}_SQ_VALU_MFMA_BUSY_CYCLES $OUT/prof_${TAG}_GRBM_GUI_ACTIVE > $OUT/prof_${TAG}_summary.log 2>&1 || exit 4
# the benchmark line LAST: profiles/traffic.json now carries this tree's kernel-source hash, so the line takes its `traffic` from it
if [ "$CFG" = "C2" ]; then python3 bench.py --full --config $CFG > $OUT/prof_${TAG}_bench.json 2> $OUT/prof_${TAG}_bench.err
else python3 bench.py --full --config $CFG --no-extras > $OUT/prof_${TAG}_bench.json 2> $OUT/prof_${TAG}_bench.err; fi
mkdir -p $OUT/prof_out
cp profiles/${TAG}_* profiles/traffic.json $OUT/prof_out/
cp $OUT/prof_${TAG}_bench.json $OUT/prof_out/${TAG}_bench.json
rm -rf $OUT/prof_${TAG}_k $OUT/prof_${TAG}_FETCH_SIZE $OUT/prof_${TAG}_WRITE_SIZE $OUT/prof_${TAG}_SQ_VALU_MFMA_BUSY_CYCLES $OUT/prof_${TAG}_GRBM_GUI_ACTIVE
echo done $TAG $CFG
