#!/bin/bash
# The runs behind DESIGN.md § mask_eqn, on one MI355X, from the repository root of a built tree:
#   profiles/r10_mask_eqn/run.sh OUT_DIR [PARENT_TREE]
# 1. profiles/hbm_bw.py (the copy bandwidth of the visit);
# 2. the 7000 x 7000 x 30 job with a QA band that is 0 on a quarter of the pixels, masked by
#    mask_eqn 'B3 != 0' and by cloudmask rasters, host and device ingest, alternating, twice;
# 3. with PARENT_TREE (a built checkout of the parent commit): the plain job and bench.py, parent
#    and this tree alternating, twice.
# Every GPU step runs under its own time limit and the script stops at the first one that fails.
set -o pipefail
O=$(realpath -m "${1:?output directory}")
HEAD=$PWD
PARENT=${2:+$(realpath "$2")}
WORK=${WORK:-/tmp/ltjob_r10}
mkdir -p "$O"
timeout -k 10 120 python profiles/hbm_bw.py 4 > "$O/hbm_bw.json" || exit 1
for i in 1 2; do
  for leg in eqn cloud; do
    for mode in host dev; do
      if [ $leg = eqn ]; then extra=(--mask-eqn 'B3 != 0'); else extra=(--qa-cloudmask); fi
      if [ $mode = dev ]; then m=(--decode device --sample device); else m=(); fi
      timeout -k 10 200 python tools/job_bench.py --mask 0.25 "${extra[@]}" "${m[@]}" \
        --work "$WORK" > "$O/job_${leg}_${mode}_$i.json" || exit 1
    done
  done
done
[ -n "$PARENT" ] || exit 0
for i in 1 2; do
  for side in parent head; do
    if [ $side = head ]; then cd "$HEAD"; else cd "$PARENT"; fi
    timeout -k 10 200 python tools/job_bench.py --work "$WORK" > "$O/plain_${side}_$i.json" || exit 1
  done
done
for i in 1 2; do
  for side in parent head; do
    if [ $side = head ]; then cd "$HEAD"; else cd "$PARENT"; fi
    timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 > "$O/bench_${side}_$i.json" || exit 1
  done
done
