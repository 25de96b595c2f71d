#!/bin/bash
# Carried-bound A/B of the F plan, one session on one box: the parent commit's library
# (lib_ab/parent/librsamd.so, RSAMD_LIB; sample, prefix and rest in every run) against this tree
# with RSAMD_CARRY=1 (prefix, rest and check in every run but a lane's first) and with
# RSAMD_CARRY=0, alternating.  Parts, in this order, all of them unless named:
#   tests  tests/test_gpu_f8_carry.py, tests/test_gpu_f8_screen.py and tests/test_gpu_f8_prune.py
#   dump   bench.py --dump-outputs of the three arms, F / inliers / record compared bit for bit
#   trace  rocprofv3 kernel trace + stats of the C2 bench, one run of its own per arm, no counters
#   ab     the plain bench.py line (--steps 100 --warmup 200), <rounds> interleaved rounds, then
#          as many at --steps 20 --warmup 5
#   probe  tools/carry_probe.py per arm: carry_stats over the 300 runs, the count between the
#          timing events
#   sweep  RSAMD_CARRY_GAP = n/50, n/25, n/16, n/10 at C2 (40 80 125 200), two rounds, the bench
#          line and the probe's fallbacks (other values: SWEEP_G="60 100")
#   c5     tools/lane_probe.py c5 (N = 10 000, 60 % outliers, 1e6 hypotheses), 3 alternating rounds
# Every GPU step runs under its own timeout and the script stops at the first failure.  Every
# line goes to bench_outputs/<tag>/ab.txt (profiles/carry/ab.txt is such a file), the traces'
# kernel statistics to bench_outputs/<tag>/trace_<arm>_kernel_stats.csv.
#   bash tools/carry_ab.sh [tag] [rounds] [part...]
set -o pipefail
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
OUT=$R/bench_outputs/${1:-carry}
N=${2:-5}
shift 2 2>/dev/null
PARTS=${*:-tests dump trace ab probe sweep c5}
PARENT=$R/tsbb15-3d-reconstruction-project_amd/lib_ab/parent/librsamd.so
[ -f $PARENT ] || { echo "no $PARENT: build the parent commit's library there first"; exit 1; }
mkdir -p $OUT
cd $R
T=$OUT/ab.txt
CFGS="parent:RSAMD_LIB=$PARENT carry:RSAMD_CARRY=1 carry0:RSAMD_CARRY=0"
has() { case " $PARTS " in *" $1 "*) return 0;; esac; return 1; }
line() {  # label steps warmup env...
  local label=$1 steps=$2 warmup=$3; shift 3
  env "$@" timeout -k 10 120 python bench.py --gpus 1 --steps $steps --warmup $warmup > $OUT/line.json 2> $OUT/line.err || { echo "$label failed"; tail -5 $OUT/line.err; return 1; }
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(json.dumps({'label':sys.argv[2],'steps':d['steps'],'warmup':d['warmup'],'value':d['value'],'ms_per_step':d['ms_per_step'],'kernels_ms':d['kernels_ms']}))" $OUT/line.json $label | tee -a $T
}
probe() {  # label env...
  local label=$1; shift
  env "$@" timeout -k 10 120 python tools/carry_probe.py $label 2> $OUT/line.err | tee -a $T || { echo "probe $label failed"; tail -5 $OUT/line.err; return 1; }
}
if has tests; then
  timeout -k 10 400 python -u -m pytest tests/test_gpu_f8_carry.py tests/test_gpu_f8_screen.py tests/test_gpu_f8_prune.py -m gpu -x -q -s > $OUT/pytest.log 2>&1
  st=$?; tail -3 $OUT/pytest.log; [ $st -eq 0 ] || exit 1
fi
if has dump; then
  for c in $CFGS; do
    env ${c#*:} timeout -k 10 120 python bench.py --gpus 1 --dump-outputs $OUT/dump_${c%%:*} > /dev/null 2> $OUT/line.err || { echo "dump ${c%%:*} failed"; tail -5 $OUT/line.err; exit 1; }
  done
  python3 tools/compare_dumps.py $OUT parent carry carry0 | tee -a $T || exit 1
fi
if has trace; then
  for c in $CFGS; do
    [ ${c%%:*} = carry0 ] && continue
    env ${c#*:} timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${c%%:*} -o bench -- python3 bench.py --gpus 1 --steps 100 --warmup 200 > $OUT/prof_${c%%:*}.log 2>&1 || { echo "trace ${c%%:*} failed"; tail -5 $OUT/prof_${c%%:*}.log; exit 1; }
    f=$(find $OUT/prof_${c%%:*} -name '*kernel_stats.csv' | head -1)
    [ -n "$f" ] || { echo "trace ${c%%:*}: no kernel statistics"; exit 1; }
    cp $f $OUT/trace_${c%%:*}_kernel_stats.csv
  done
fi
if has ab; then
  for sw in "100 200" "20 5"; do
    for i in $(seq $N); do
      for c in $CFGS; do line ${c%%:*} $sw ${c#*:} || exit 1; done
    done
  done
fi
if has probe; then
  for c in $CFGS; do probe ${c%%:*} ${c#*:} || exit 1; done
fi
if has sweep; then
  for i in 1 2; do
    for g in ${SWEEP_G:-40 80 125 200}; do
      line carry_gap$g 100 200 RSAMD_CARRY=1 RSAMD_CARRY_GAP=$g || exit 1
      probe carry_gap$g RSAMD_CARRY=1 RSAMD_CARRY_GAP=$g || exit 1
    done
  done
fi
if has c5; then
  for i in 1 2 3; do
    for c in $CFGS; do
      [ ${c%%:*} = carry0 ] && continue
      env ${c#*:} timeout -k 10 120 python tools/lane_probe.py c5 ${c%%:*} | tee -a $T || exit 1
    done
  done
fi
