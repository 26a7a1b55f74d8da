#!/bin/bash
# usage (GPU box): tools/ab_pair.sh "<configs>" [reps] [arms...]  -- interleaved A/B on ONE device of the paired main-pass
# kernel (bf16_filter_kernel_pair), one line per run.  Arms: parent = a parent build's library ($PN_PARENT_LIB, a path
# relative to the repository root), w4 = this build with --waves 4, auto = this build's own choice, anything else = the
# diagnostic library of that tag on its own choice (stagger arms: PN_DIAG_TAG=stag0 PN_DIAG_FLAGS="-DPN_DIAG_PAIR_STAGGER=0",
# stag2 likewise with 2: both halves in one placement / the lagging half a whole chain behind).
# PN_AB_STEPS / PN_AB_WARMUP: bench steps (20 / 5); PN_AB_FULL=1: with the parity leg (--full).
ROOT=$(cd "$(dirname "$0")/.." && pwd)  # the repository root: this script lives in tools/
cd $ROOT
OUT=${OUT:-tools_out}  # output folder, relative to the repository root
mkdir -p $OUT
CFGS=${1:-c2}; R=${2:-5}
[ $# -ge 2 ] && shift 2 || shift $#
ARMS=${@:-parent w4 auto}
case " $ARMS " in *" parent "*)
  [ -n "$PN_PARENT_LIB" ] && [ -f "$ROOT/$PN_PARENT_LIB" ] || { echo "usage: PN_PARENT_LIB=<a parent build's library, relative to the repository root> $0 \"<configs>\" [reps] [arms...]  (the parent arm needs it)" >&2; exit 2; };;
esac
MODE="--no-verify"; [ "${PN_AB_FULL:-0}" = 1 ] && MODE="--full"
for c in $CFGS; do
  for rep in $(seq 1 $R); do
    for v in $ARMS; do
      unset PN_LIBRARY_PATH PN_LIBRARY_OLDER; W=0
      case $v in
        parent) export PN_LIBRARY_PATH=$ROOT/$PN_PARENT_LIB PN_LIBRARY_OLDER=1;;
        w4) W=4;;
        auto) ;;
        *) export PN_LIBRARY_PATH=$ROOT/petal-neighbors_amd/libpetal_mi355x_diag_$v.so;;
      esac
      timeout -k 10 300 python bench.py --gpus 1 $MODE --no-cpu-baseline --steps ${PN_AB_STEPS:-20} --warmup ${PN_AB_WARMUP:-5} --config $c --waves $W > $OUT/abp_$v.json 2> $OUT/abp_$v.err || { echo "$c $v failed"; tail -3 $OUT/abp_$v.err; exit 1; }
      python3 -c "
import json
d=json.loads([l for l in open('$OUT/abp_$v.json') if l.startswith('{')][-1]); r=d['roofline']
print('%-6s %-6s steps ${PN_AB_STEPS:-20} rep $rep step %.4f kernel ms/step %.4f  cand/q %.1f eval/q %.1f fb %d verified %s' % ('$c', '$v', d['ms_per_step'], r['kernel_ms_per_step'], d['candidates_per_query'], d['exact_evaluations_per_query'], d['fallback_queries'], d.get('verified')))
"
    done
  done
done
