#!/bin/bash
# usage: bash tools/gpu_merge_bins.sh [build] VARIANT... -- tk_k_merge_all in builds with timing hooks (wrong tokens: timing only).  A variant
# is a name of words joined by "+": binB = -DTKM_ONLY_BIN=B (only length bin B is merged), noprobes = -DTKM_NO_PROBES=1, onestep =
# -DTKM_ONE_STEP=1 (one merge per step), all = the shipped library; e.g. `all bin0 bin8 bin8+onestep`.  The variants are made with
# tools/build_variant.sh (`build` rebuilds them; a run builds those it does not find) and selected with $TIKTOKEN_AMD_LIB.  The series
# stops at the first variant that fails.  Results in $OUT/mbins/out.txt ($OUT: out/ by default, relative to the repository root).
R=$(cd "$(dirname "$0")/.." && pwd)
MODE=; [ "$1" = build ] && { MODE=build; shift; }
flags() {
  local w f=
  for w in ${1//+/ }; do
    case $w in
      all) ;;
      bin[0-9]*) f="$f -DTKM_ONLY_BIN=${w#bin}" ;;
      noprobes) f="$f -DTKM_NO_PROBES=1" ;;
      onestep) f="$f -DTKM_ONE_STEP=1" ;;
      *) echo "unknown variant word: $w" >&2; return 1 ;;
    esac
  done
  echo $f
}
V_DIR=$R/tiktoken_amd/csrc/variants; mkdir -p $V_DIR
lib() { [ "$1" != all ] && echo $V_DIR/libtiktoken_amd_$1.so; }
for V in "$@"; do F=$(flags $V) || exit 1; done
for V in "$@"; do
  L=$(lib $V) && { [ "$MODE" = build ] || [ ! -f $L ]; } && { rm -f $L; bash $R/tools/build_variant.sh $V $(flags $V) > $V_DIR/$V.build.log 2>&1 & }
done; wait
for V in "$@"; do L=$(lib $V) && { [ -f $L ] || { echo "variant $V did not build: $V_DIR/$V.build.log"; exit 1; }; }; done
[ "$MODE" = build ] && exit 0
cd $R; OUT=${OUT:-out}; mkdir -p $OUT/mbins; : > $OUT/mbins/out.txt
for V in "$@"; do
  TIKTOKEN_AMD_LIB=$(lib $V) timeout 120 python tools/exp_front.py --tag $V --steps 2 --no-parity 2>/dev/null | grep '^EXP ' | sed 's/^EXP //' | python -c "
import sys, json
j = json.loads(sys.stdin.read()); print('variant', '$V', 'merge_all ms', j['kernels_ms'].get('tk_k_merge_all'), 'step', j['ms_per_step'])" >> $OUT/mbins/out.txt
  [ ${PIPESTATUS[0]} = 0 ] || { echo "variant $V failed"; break; }
done
cat $OUT/mbins/out.txt
