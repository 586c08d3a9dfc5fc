#!/bin/bash
# usage: bash tools/gpu_phases.sh TAG | build -- per-phase cost of tk_k_front: builds of the library that stop the kernel after each phase
# (-DTKF_STOP_AFTER=1 .. 5: nothing behind the front kernel runs then, tk_api.hip stage_back `front_only`; -DTKF_PROBE_LEN=1: every probe
# answered without a table access), made with tools/build_variant.sh and selected with $TIKTOKEN_AMD_LIB; debug bit 8 on the shipped library:
# pieces that are not tokens are not claimed.  `build` (re)builds the variants, on any machine; a run builds those it does not find.  Timed
# with the library's HIP events; SQ_INSTS_* counted in one rocprofv3 --pmc pass per variant.  The series stops at the first variant that
# fails (a faulting kernel can leave the box unusable).  Results under $OUT/phases_TAG ($OUT: out/ by default, relative to the repository root).
R=$(cd "$(dirname "$0")/.." && pwd)
declare -A FLAG=([stopA]=-DTKF_STOP_AFTER=1 [stopB]=-DTKF_STOP_AFTER=2 [stopC]=-DTKF_STOP_AFTER=3 [stopD]=-DTKF_STOP_AFTER=4 [stopE]=-DTKF_STOP_AFTER=5
                 [probelen]=-DTKF_PROBE_LEN=1)
declare -A DBG=([starts_only]=8)
VARS=${VARIANTS:-all stopA stopB stopC stopD stopE probelen starts_only}
V_DIR=$R/tiktoken_amd/csrc/variants; mkdir -p $V_DIR
lib() { [ -n "${FLAG[$1]}" ] && echo $V_DIR/libtiktoken_amd_$1.so; }
for V in $VARS; do
  L=$(lib $V) && { [ "$1" = build ] || [ ! -f $L ]; } && { rm -f $L; bash $R/tools/build_variant.sh $V ${FLAG[$V]} > $V_DIR/$V.build.log 2>&1 & }
done; wait
for V in $VARS; do L=$(lib $V) && { [ -f $L ] || { echo "variant $V did not build: $V_DIR/$V.build.log"; exit 1; }; }; done
[ "$1" = build ] && exit 0
TAG=${1:-r02}
OUT=${OUT:-out}; O=$(cd $R && mkdir -p $OUT/phases_$TAG && cd $OUT/phases_$TAG && pwd)
cd /tmp && export TMPDIR=/tmp
for V in $VARS; do
  TIKTOKEN_AMD_LIB=$(lib $V) TIKTOKEN_AMD_DEBUG=${DBG[$V]:-0} timeout 90 python $R/bench.py --full --gpus 1 --steps 2 --warmup 1 --mib 1024 --no-cpu-baseline --no-host-path > $O/bench_$V.json 2> $O/bench_$V.err || { echo "variant $V failed: $(tail -2 $O/bench_$V.err)"; fail=1; break; }
done
[ -n "$fail" ] || for V in ${PMC_VARIANTS:-$VARS}; do
  [ -s $O/bench_$V.json ] || continue
  TIKTOKEN_AMD_LIB=$(lib $V) TIKTOKEN_AMD_DEBUG=${DBG[$V]:-0} timeout 150 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU --output-format csv -d $O/pmc_$V -o p -- python $R/bench.py --gpus 1 --steps 1 --warmup 0 --mib 1024 --no-cpu-baseline --no-host-path > $O/pmc_$V.log 2>&1 || { echo "pmc pass $V failed"; fail=1; break; }
done
cd $R; python - "$O" $VARS <<'PY'
import csv, glob, json, os, sys, collections
O = sys.argv[1]
print("variant,front_ms,all_kernels_ms,VALU,SALU,LDS,VMEM_RD,WAVE_CYCLES,WAIT_ANY,WAIT_INST_ANY,ACTIVE_VALU")
for V in sys.argv[2:]:
    try:
        j = json.loads(open(f"{O}/bench_{V}.json").read().strip().splitlines()[-1])
        fm = j["roofline"]["kernels_ms_avg"].get("tk_k_front"); am = j["roofline"]["all_kernels_ms_per_step"]
    except Exception as e:
        fm = am = None
    agg = collections.defaultdict(list)
    for f in glob.glob(f"{O}/pmc_{V}/**/p_counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "tk_k_front<" in r["Kernel_Name"] and r["Kernel_Name"].split("(")[0].replace(" ", "").endswith(",0>"):
                agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
    g = lambda c: ("%.0f" % max(agg[c])) if agg.get(c) else ""
    print(",".join(map(str, [V, fm, am, g("SQ_INSTS_VALU"), g("SQ_INSTS_SALU"), g("SQ_INSTS_LDS"), g("SQ_INSTS_VMEM_RD"), g("SQ_WAVE_CYCLES"), g("SQ_WAIT_ANY"), g("SQ_WAIT_INST_ANY"), g("SQ_ACTIVE_INST_VALU")])))
PY
find $O -name '*.csv' -size +5M -delete
[ -z "$fail" ]
