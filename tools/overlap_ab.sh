#!/bin/bash
# Lane A/B of the F plan, one session on one box (the ranges of one session are what counts,
# DESIGN.md §4): the lane tests, then alternating the parent commit's library (if
# lib_ab/parent/librsamd.so exists; RSAMD_LIB), two lanes (RSAMD_OVERLAP=1) and one lane
# (RSAMD_OVERLAP=0)
#   1. the plain bench.py line at the default flags and at the driver's (--steps 20 --warmup 5),
#      <rounds> times each, and once with --dump-outputs (F / inliers / record compared);
#   2. two lanes with RSAMD_QSLICES = 1, 2, 3 (plain line, default flags), 3 rounds;
#   3. tools/lane_probe.py: timing level 0, runs in batches of 3 with a result() between, and
#      the c5_stress leg alone, <rounds> times each.
# Every line goes to bench_outputs/<tag>/ab.txt (profiles/lanes/ab.txt is one such file).
#   bash tools/overlap_ab.sh [tag] [rounds]
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/bench_outputs/${1:-lanes}
N=${2:-5}
PARENT=$R/tsbb15-3d-reconstruction-project_amd/lib_ab/parent/librsamd.so
mkdir -p $OUT
cd $R
timeout -k 10 300 python -u -m pytest tests/test_gpu_lanes.py tests/test_gpu_overlap.py -m gpu -x -q > $OUT/pytest.log 2>&1
st=$?; tail -2 $OUT/pytest.log; [ $st -eq 0 ] || exit 1
T=$OUT/ab.txt
: > $T
CFGS="lanes2:RSAMD_OVERLAP=1 lanes1:RSAMD_OVERLAP=0"
[ -f $PARENT ] && CFGS="parent:RSAMD_LIB=$PARENT $CFGS"
line() {  # label steps warmup env...
  local label=$1 steps=$2 warm=$3; shift 3
  env "$@" timeout -k 10 120 python bench.py --gpus 1 --steps $steps --warmup $warm > $OUT/line.json 2> $OUT/line.err || { echo "$label failed"; tail -5 $OUT/line.err; return 1; }
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(json.dumps({'label':sys.argv[2],'steps':d['steps'],'warmup':d['warmup'],'value':d['value'],'ms_per_step':d['ms_per_step'],'kernels_ms':d['kernels_ms']}))" $OUT/line.json $label | tee -a $T
}
# results unchanged: the last timed step's outputs, array for array
for c in $CFGS; do
  env ${c#*:} timeout -k 10 120 python bench.py --gpus 1 --dump-outputs $OUT/dump_${c%%:*} > /dev/null 2> $OUT/line.err || { echo "dump ${c%%:*} failed"; tail -5 $OUT/line.err; exit 1; }
done
python3 - $OUT $CFGS <<'EOF' | tee -a $T || exit 1
import os, sys
import numpy as np
out, labels = sys.argv[1], [c.split(":")[0] for c in sys.argv[2:]]
ok = True
for lab in labels[1:]:
    for f in ("F.npy", "inliers.npy", "record.npy"):
        a = np.load(os.path.join(out, "dump_" + labels[0], f))
        b = np.load(os.path.join(out, "dump_" + lab, f))
        eq = a.shape == b.shape and a.tobytes() == b.tobytes()
        ok &= eq
        print(f"dump {labels[0]} vs {lab}: {f} shape {a.shape} equal={eq}")
sys.exit(0 if ok else 1)
EOF
for flags in "100 200" "20 5"; do
  for i in $(seq $N); do
    for c in $CFGS; do line ${c%%:*} $flags ${c#*:} || exit 1; done
  done
done
for i in 1 2 3; do
  for q in 1 2 3; do line lanes2_qslices$q 100 200 RSAMD_OVERLAP=1 RSAMD_QSLICES=$q || exit 1; done
done
for probe in timing0 batch c5; do
  for i in $(seq $N); do
    for c in $CFGS; do
      env ${c#*:} timeout -k 10 120 python tools/lane_probe.py $probe ${c%%:*} | tee -a $T || exit 1
    done
  done
done
