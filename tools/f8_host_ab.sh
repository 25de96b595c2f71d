#!/bin/bash
# A/B of the whole library against another build of it (profiles/f8_host/ab.txt, after the protocol
# of profiles/host_layer/ab.txt): per round and side one bench.py --full and one
# tools/plan_create_probe.py, each a fresh process, one at a time, the side that runs first
# alternating.  Usage: bash tools/f8_host_ab.sh <parent librsamd.so> <rounds> <first round> <out file>
# Every JSON line goes to <out file> behind its label; stops at the first run that fails.
set -o pipefail
PARENT=$(readlink -f "$1"); ROUNDS=$2; FIRST=$3; OUT=$4
cd "$(dirname "$0")/.."
one() {  # label, library ("" = this tree's)
  local env=(); [ -n "$2" ] && env=(RSAMD_LIB="$2")
  env "${env[@]}" timeout -k 10 300 python3 bench.py --gpus 1 --full --no-cpu-baseline --no-fp64-count \
      --no-split-projection | tail -n 1 | sed "s/^/$1 /" >> "$OUT" || return 1
  env "${env[@]}" timeout -k 10 120 python3 tools/plan_create_probe.py --label "$1" | sed "s/^/$1 /" >> "$OUT" || return 1
  echo "round $r $1 done"
}
for ((r = FIRST; r < FIRST + ROUNDS; ++r)); do
  if ((r % 2 == 0)); then one parent "$PARENT" && one new "" || exit 1
  else one new "" && one parent "$PARENT" || exit 1; fi
done
