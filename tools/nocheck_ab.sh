#!/bin/bash
# A/B of the F plan without the check launch (a carried run is prefix and rest; a run that fell back
# is counted again at the flush that reads it), one session on one box: the parent commit's library
# (lib_ab/parent/librsamd.so, RSAMD_LIB, built there by tools/build_ab.sh from the parent commit;
# prefix, rest and check in every carried run) against this tree, alternating.  Parts, in this
# order, all of them unless named:
#   tests  tests/test_gpu_f8_recount.py, test_gpu_f8_carry.py, test_gpu_f8_screen.py,
#          test_gpu_f8_prune.py and test_gpu_lanes.py
#   dump   bench.py --dump-outputs of both arms, F / inliers / record compared bit for bit
#   trace  rocprofv3 kernel trace + stats of the C2 bench, one run of its own per arm, no counters;
#          the new arm's statistics must not name k_f8_count32q<256, 3>
#   ab     the plain bench.py line (--steps 100 --warmup 200), <rounds> interleaved rounds, then as
#          many at --steps 20 --warmup 5; then the verdict: medians, the ratio, and whether every
#          line of the new arm is above every line of the parent arm at --steps 100 --warmup 200
#   probe  tools/carry_probe.py per arm: fallbacks, recounts and lane_waits over the 300 runs (all 0
#          in the new arm, or the part fails), the count between the timing events
#   c5     tools/lane_probe.py c5 (N = 10 000, 60 % outliers, 1e6 hypotheses), 3 alternating rounds
#   chain  tools/chain_probe.py per arm, 2 alternating rounds: wall time per run at H = 1e5, 5e4,
#          2.5e4 and 4096 (the floor of the launch chain, where the removed launch shows in full)
# Every GPU step runs under its own timeout and the script stops at the first failure.  Every
# line goes to bench_outputs/<tag>/ab.txt (profiles/nocheck/ab.txt is such a file), the traces'
# kernel statistics to bench_outputs/<tag>/trace_<arm>_kernel_stats.csv.
#   bash tools/nocheck_ab.sh [tag] [rounds] [part...]
set -o pipefail
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
OUT=$R/bench_outputs/${1:-nocheck}
N=${2:-5}
shift 2 2>/dev/null
PARTS=${*:-tests dump trace ab probe c5 chain}
PARENT=$R/tsbb15-3d-reconstruction-project_amd/lib_ab/parent/librsamd.so
[ -f $PARENT ] || { echo "no $PARENT: build the parent commit's library there first"; exit 1; }
mkdir -p $OUT
cd $R
T=$OUT/ab.txt
CFGS="parent:RSAMD_LIB=$PARENT nocheck:RSAMD_CARRY=1"
has() { case " $PARTS " in *" $1 "*) return 0;; esac; return 1; }
line() {  # label steps warmup env...
  local label=$1 steps=$2 warmup=$3; shift 3
  env "$@" timeout -k 10 120 python bench.py --gpus 1 --steps $steps --warmup $warmup > $OUT/line.json 2> $OUT/line.err || { echo "$label failed"; tail -5 $OUT/line.err; return 1; }
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(json.dumps({'label':sys.argv[2],'steps':d['steps'],'warmup':d['warmup'],'value':d['value'],'ms_per_step':d['ms_per_step'],'kernels_ms':d['kernels_ms']}))" $OUT/line.json $label | tee -a $T
}
if has tests; then
  timeout -k 10 500 python -u -m pytest tests/test_gpu_f8_recount.py tests/test_gpu_f8_carry.py tests/test_gpu_f8_screen.py tests/test_gpu_f8_prune.py tests/test_gpu_lanes.py -m gpu -x -q -s --durations=12 > $OUT/pytest.log 2>&1
  st=$?; tail -3 $OUT/pytest.log; [ $st -eq 0 ] || exit 1
fi
if has dump; then
  for c in $CFGS; do
    env ${c#*:} timeout -k 10 120 python bench.py --gpus 1 --dump-outputs $OUT/dump_${c%%:*} > /dev/null 2> $OUT/line.err || { echo "dump ${c%%:*} failed"; tail -5 $OUT/line.err; exit 1; }
  done
  python3 tools/compare_dumps.py $OUT parent nocheck | tee -a $T || exit 1
fi
if has trace; then
  for c in $CFGS; do
    env ${c#*:} timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${c%%:*} -o bench -- python3 bench.py --gpus 1 --steps 100 --warmup 200 > $OUT/prof_${c%%:*}.log 2>&1 || { echo "trace ${c%%:*} failed"; tail -5 $OUT/prof_${c%%:*}.log; exit 1; }
    f=$(find $OUT/prof_${c%%:*} -name '*kernel_stats.csv' | head -1)
    [ -n "$f" ] || { echo "trace ${c%%:*}: no kernel statistics"; exit 1; }
    cp $f $OUT/trace_${c%%:*}_kernel_stats.csv
  done
  if grep -q 'k_f8_count32q<256, 3>' $OUT/trace_nocheck_kernel_stats.csv; then
    echo "trace nocheck: the check launch is still there" | tee -a $T; exit 1
  fi
  echo "trace nocheck: no k_f8_count32q<256, 3>" | tee -a $T
fi
if has ab; then
  for sw in "100 200" "20 5"; do
    for i in $(seq $N); do
      for c in $CFGS; do line ${c%%:*} $sw ${c#*:} || exit 1; done
    done
  done
  python3 - $T <<'EOF' | tee -a $T
import json, statistics, sys
rows = [json.loads(l) for l in open(sys.argv[1]) if l.startswith('{"label"') and '"probe"' not in l]
for steps, warmup in ((100, 200), (20, 5)):
    v = {a: [r["value"] for r in rows if r["label"] == a and r["steps"] == steps and r["warmup"] == warmup]
         for a in ("parent", "nocheck")}
    if not v["parent"] or not v["nocheck"]:
        continue
    med = {a: statistics.median(x) for a, x in v.items()}
    clear = min(v["nocheck"]) > max(v["parent"])
    print(json.dumps({"verdict": f"steps {steps} warmup {warmup}", "rounds": len(v["nocheck"]),
                      "parent": [min(v["parent"]), med["parent"], max(v["parent"])],
                      "nocheck": [min(v["nocheck"]), med["nocheck"], max(v["nocheck"])],
                      "ratio_of_medians": med["nocheck"] / med["parent"],
                      "every_nocheck_line_above_every_parent_line": clear}))
EOF
fi
if has probe; then
  for c in $CFGS; do
    env ${c#*:} timeout -k 10 120 python tools/carry_probe.py ${c%%:*} 2> $OUT/line.err | tee $OUT/probe_${c%%:*}.json | tee -a $T || { echo "probe ${c%%:*} failed"; tail -5 $OUT/line.err; exit 1; }
  done
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);ok=d['carry_stats']['fallbacks']==0 and d['recount_stats'][0]==0 and d['lane_waits']==0 and d['recount_stats'][1]==2;print('probe nocheck: fallbacks, recounts, lane_waits 0 and two count launches:',ok);sys.exit(0 if ok else 1)" $OUT/probe_nocheck.json | tee -a $T || exit 1
fi
if has c5; then
  for i in 1 2 3; do
    for c in $CFGS; do
      env ${c#*:} timeout -k 10 120 python tools/lane_probe.py c5 ${c%%:*} | tee -a $T || exit 1
    done
  done
fi
if has chain; then
  for i in 1 2; do
    for c in $CFGS; do
      env ${c#*:} timeout -k 10 120 python tools/chain_probe.py ${c%%:*} | tee -a $T || exit 1
    done
  done
fi
