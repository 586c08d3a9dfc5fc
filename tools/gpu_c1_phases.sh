#!/bin/bash
# usage: bash tools/gpu_c1_phases.sh [build] -- C1 (1 MiB of Lorem ipsum, one document, gpt2-shaped): the front kernel stopped after each phase
# (builds with -DTKF_STOP_AFTER=1 .. 5), without probes (-DTKF_PROBE_LEN=1), without claims (debug bit 8), without the in-call table (256).
# The variants are made with tools/build_variant.sh (`build` rebuilds them; a run builds those it does not find) and selected with
# $TIKTOKEN_AMD_LIB.  The series stops at the first variant that fails.
R=$(cd "$(dirname "$0")/.." && pwd)
declare -A FLAG=([stopA]=-DTKF_STOP_AFTER=1 [stopB]=-DTKF_STOP_AFTER=2 [stopC]=-DTKF_STOP_AFTER=3 [stopD]=-DTKF_STOP_AFTER=4 [stopE]=-DTKF_STOP_AFTER=5
                 [probelen]=-DTKF_PROBE_LEN=1)
declare -A DBG=([starts_only]=8 [no_mt]=256)
VARS="all stopA stopB stopC stopD stopE probelen starts_only no_mt"
V_DIR=$R/tiktoken_amd/csrc/variants; mkdir -p $V_DIR
lib() { [ -n "${FLAG[$1]}" ] && echo $V_DIR/libtiktoken_amd_$1.so; }
for V in $VARS; do
  L=$(lib $V) && { [ "$1" = build ] || [ ! -f $L ]; } && { rm -f $L; bash $R/tools/build_variant.sh $V ${FLAG[$V]} > $V_DIR/$V.build.log 2>&1 & }
done; wait
for V in $VARS; do L=$(lib $V) && { [ -f $L ] || { echo "variant $V did not build: $V_DIR/$V.build.log"; exit 1; }; }; done
[ "$1" = build ] && exit 0
cd $R
for V in $VARS; do
  TIKTOKEN_AMD_LIB=$(lib $V) TIKTOKEN_AMD_DEBUG=${DBG[$V]:-0} timeout 100 python tools/bench_configs.py C1 2>/dev/null | python -c "
import sys, json
for l in sys.stdin:
    j = json.loads(l); k = j['kernels_ms_avg']
    print('%-11s: %.3f ms per step, front %.4f place %.4f merge %.4f count %.4f scan %.4f  sum %.3f  parity %s' % ('$V', j['ms_per_step'], k.get('tk_k_front', 0), k.get('tk_k_place', 0), k.get('tk_k_merge_all', 0), k.get('tk_k_count_tiles', 0), k.get('tk_k_scan_small', 0), sum(k.values()), j['parity_all_tokens']))
"
  [ ${PIPESTATUS[0]} = 0 ] || { echo "variant $V failed"; break; }
done
