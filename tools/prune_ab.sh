#!/bin/bash
# Pruned-count A/B of the F plan, one session on one box: alternating the parent commit's
# library (lib_ab/parent/librsamd.so, RSAMD_LIB), this tree with RSAMD_PRUNE=0 (one whole-window
# counting launch) and with RSAMD_PRUNE=1 (sample -> prefix -> rest).  Parts, in this order,
# all of them unless named:
#   tests  tests/test_gpu_f8_prune.py
#   dump   bench.py --dump-outputs of every arm, F / inliers / record compared with the parent's
#   ab     the plain bench.py line (--steps 100 --warmup 200), <rounds> interleaved rounds
#   sweep  RSAMD_PRUNE_MARGIN and RSAMD_PRUNE_SAMPLE around the defaults at C2, 2 rounds
#   c5     tools/lane_probe.py c5 (N = 10 000, 60 % outliers, 1e6 hypotheses) alone, <rounds> rounds
# Every line goes to bench_outputs/<tag>/ab.txt (profiles/prune/ab.txt is such a file).
#   bash tools/prune_ab.sh [tag] [rounds] [part...]
set -o pipefail
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
OUT=$R/bench_outputs/${1:-prune}
N=${2:-5}
shift 2 2>/dev/null
PARTS=${*:-tests dump ab sweep c5}
PARENT=$R/tsbb15-3d-reconstruction-project_amd/lib_ab/parent/librsamd.so
mkdir -p $OUT
cd $R
T=$OUT/ab.txt
CFGS="prune0:RSAMD_PRUNE=0 prune1:RSAMD_PRUNE=1"
[ -f $PARENT ] && CFGS="parent:RSAMD_LIB=$PARENT $CFGS"
has() { case " $PARTS " in *" $1 "*) return 0;; esac; return 1; }
line() {  # label env...
  local label=$1; shift
  env "$@" timeout -k 10 120 python bench.py --gpus 1 --steps 100 --warmup 200 > $OUT/line.json 2> $OUT/line.err || { echo "$label failed"; tail -5 $OUT/line.err; return 1; }
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(json.dumps({'label':sys.argv[2],'steps':d['steps'],'warmup':d['warmup'],'value':d['value'],'ms_per_step':d['ms_per_step'],'kernels_ms':d['kernels_ms']}))" $OUT/line.json $label | tee -a $T
}
if has tests; then
  timeout -k 10 300 python -u -m pytest tests/test_gpu_f8_prune.py -m gpu -x -q -s > $OUT/pytest.log 2>&1
  st=$?; tail -3 $OUT/pytest.log; [ $st -eq 0 ] || exit 1
fi
if has dump; then
  for c in $CFGS; do
    env ${c#*:} timeout -k 10 120 python bench.py --gpus 1 --dump-outputs $OUT/dump_${c%%:*} > /dev/null 2> $OUT/line.err || { echo "dump ${c%%:*} failed"; tail -5 $OUT/line.err; exit 1; }
  done
  python3 tools/compare_dumps.py $OUT $(for c in $CFGS; do echo ${c%%:*}; done) | tee -a $T || exit 1
fi
if has ab; then
  for i in $(seq $N); do
    for c in $CFGS; do line ${c%%:*} ${c#*:} || exit 1; done
  done
fi
if has sweep; then
  for i in 1 2; do
    for m in 50 75 100 150 200; do line prune1_margin$m RSAMD_PRUNE=1 RSAMD_PRUNE_MARGIN=$m || exit 1; done
    for g in 8 16 32; do line prune1_sample$g RSAMD_PRUNE=1 RSAMD_PRUNE_SAMPLE=$g || exit 1; done
  done
fi
if has c5; then
  for i in $(seq $N); do
    for c in $CFGS; do
      env ${c#*:} timeout -k 10 120 python tools/lane_probe.py c5 ${c%%:*} | tee -a $T || exit 1
    done
  done
fi
