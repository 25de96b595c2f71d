#!/bin/bash
# A/B of the F plan's point order (the winner's outliers first in the pruned count's copies of the
# points), one session on one box: the parent commit's library (lib_ab/parent/librsamd.so,
# RSAMD_LIB, built there by tools/build_ab.sh from the parent commit) against this tree and against
# this tree with RSAMD_ORDER=0, alternating.  Parts, in this order, all of them unless named:
#   dump   bench.py --dump-outputs of the three arms, F / inliers / record compared bit for bit
#   trace  rocprofv3 kernel trace + stats of the C2 bench, one run of its own per arm (parent,
#          order), no counters
#   ab     the plain bench.py line (--steps 100 --warmup 200), <rounds> interleaved rounds of
#          parent / order / order0, then as many at --steps 20 --warmup 5; then the verdict: the
#          ranges, the ratio of medians, whether every line of the new arm is above every line of
#          the parent arm and whether RSAMD_ORDER=0 lies inside the parent's range
#   probe  tools/carry_probe.py per arm: prune_stats (the survivors) and order_stats of the last
#          run, fallbacks, recounts, lane_waits (0 in the new arm, two count launches, or the part
#          fails), the count between the timing events
#   c5     tools/lane_probe.py c5 (N = 10 000, 60 % outliers, 1e6 hypotheses), 3 alternating rounds
#   chain  tools/chain_probe.py per arm, 2 alternating rounds: wall time per run at H = 1e5, 5e4,
#          2.5e4 and 4096
#   sweep  this tree with the order on, the bench line, 2 rounds each: the margin m = 16, n/60,
#          n/30, n/20, n/15 (RSAMD_PRUNE_MARGIN) and 1, 2, 3, 4 slices per resident wave (RSAMD_QSLICES)
# Every GPU step runs under its own timeout and the script stops at the first failure.  Every
# line goes to bench_outputs/<tag>/ab.txt (profiles/order/ab.txt is such a file), the traces'
# kernel statistics to bench_outputs/<tag>/trace_<arm>_kernel_stats.csv.
#   bash tools/order_ab.sh [tag] [rounds] [part...]
set -o pipefail
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
OUT=$R/bench_outputs/${1:-order}
N=${2:-5}
shift 2 2>/dev/null
PARTS=${*:-dump trace ab probe c5 chain sweep}
PARENT=$R/tsbb15-3d-reconstruction-project_amd/lib_ab/parent/librsamd.so
[ -f $PARENT ] || { echo "no $PARENT: build the parent commit's library there first"; exit 1; }
mkdir -p $OUT
cd $R
T=$OUT/ab.txt
CFGS="parent:RSAMD_LIB=$PARENT order:RSAMD_ORDER=1 order0:RSAMD_ORDER=0"
has() { case " $PARTS " in *" $1 "*) return 0;; esac; return 1; }
line() {  # label steps warmup env...
  local label=$1 steps=$2 warmup=$3; shift 3
  env "$@" timeout -k 10 120 python bench.py --gpus 1 --steps $steps --warmup $warmup > $OUT/line.json 2> $OUT/line.err || { echo "$label failed"; tail -5 $OUT/line.err; return 1; }
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(json.dumps({'label':sys.argv[2],'steps':d['steps'],'warmup':d['warmup'],'value':d['value'],'ms_per_step':d['ms_per_step'],'kernels_ms':d['kernels_ms']}))" $OUT/line.json $label | tee -a $T
}
if has dump; then
  for c in $CFGS; do
    env ${c#*:} timeout -k 10 120 python bench.py --gpus 1 --dump-outputs $OUT/dump_${c%%:*} > /dev/null 2> $OUT/line.err || { echo "dump ${c%%:*} failed"; tail -5 $OUT/line.err; exit 1; }
  done
  python3 tools/compare_dumps.py $OUT parent order | tee -a $T || exit 1
  python3 tools/compare_dumps.py $OUT parent order0 | tee -a $T || exit 1
fi
if has trace; then
  for c in $CFGS; do
    [ ${c%%:*} = order0 ] && continue
    env ${c#*:} timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${c%%:*} -o bench -- python3 bench.py --gpus 1 --steps 100 --warmup 200 > $OUT/prof_${c%%:*}.log 2>&1 || { echo "trace ${c%%:*} failed"; tail -5 $OUT/prof_${c%%:*}.log; exit 1; }
    f=$(find $OUT/prof_${c%%:*} -name '*kernel_stats.csv' | head -1)
    [ -n "$f" ] || { echo "trace ${c%%:*}: no kernel statistics"; exit 1; }
    cp $f $OUT/trace_${c%%:*}_kernel_stats.csv
    grep -E 'k_f8_count32q|k_f8_tail_solve|k_pack_points32q_perm' $f | sed "s/^/trace ${c%%:*}: /" | tee -a $T
  done
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
         for a in ("parent", "order", "order0")}
    if not all(v.values()):
        continue
    med = {a: statistics.median(x) for a, x in v.items()}
    print(json.dumps({"verdict": f"steps {steps} warmup {warmup}", "rounds": len(v["order"]),
                      **{a: [min(x), med[a], max(x)] for a, x in v.items()},
                      "ratio_of_medians": med["order"] / med["parent"],
                      "every_order_line_above_every_parent_line": min(v["order"]) > max(v["parent"]),
                      "order0_inside_parent_range":
                          min(v["parent"]) <= min(v["order0"]) and max(v["order0"]) <= max(v["parent"])}))
EOF
fi
if has probe; then
  for c in $CFGS; do
    env ${c#*:} timeout -k 10 120 python tools/carry_probe.py ${c%%:*} 2> $OUT/line.err | tee $OUT/probe_${c%%:*}.json | tee -a $T || { echo "probe ${c%%:*} failed"; tail -5 $OUT/line.err; exit 1; }
  done
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);ok=d['carry_stats']['fallbacks']==0 and d['recount_stats'][0]==0 and d['lane_waits']==0 and d['recount_stats'][1]==2 and d['order_stats']['installed'] and d['order_stats']['installs']==1;print('probe order: installed once, fallbacks, recounts, lane_waits 0 and two count launches:',ok);sys.exit(0 if ok else 1)" $OUT/probe_order.json | tee -a $T || exit 1
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
if has sweep; then
  for i in 1 2; do
    for m in 16 33 66 100 133; do line order_m$m 100 200 RSAMD_PRUNE_MARGIN=$m || exit 1; done
    for q in 1 2 3 4; do line order_q$q 100 200 RSAMD_QSLICES=$q || exit 1; done
  done
fi
