#!/bin/bash
# Alternating A/B of the edge-pass instruction-count forms on one box, in the style of profiles/class_tail/ab.sh.
# usage (from the repository root): ab.sh <rounds> <checkout of the parent commit, built>
# Every round runs the parent, this build, and this build with DGCNN_EDGE_VALU=0; one line per run:
#   <name> <ms_per_step (median region)> <fastest region>
here=$PWD
rounds=$1; parent=$2
run() {   # name, directory, environment
  ms=$(cd "$2" && env $3 timeout -k 10 240 python bench.py --full --no-cpu-baseline --no-edgeconv-stack 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], min(d['config']['per_repeat_ms_per_step']))") || return 1
  echo "$1 $ms"
}
for rep in $(seq $rounds); do
  run parent "$parent" X=0 || exit 1
  run this "$here" X=0 || exit 1
  run this_switch_off "$here" DGCNN_EDGE_VALU=0 || exit 1
done
