#!/bin/bash
# Round 6: the GPU suite and the round's profiles on the final code -- tests (with the log of the reference-package / Appendix-B files), smoke, kernel stats + HBM
# traffic, SQ counters, the front kernel by phase (instruction counters and cycles per tile), bench line, configs, link rates, host path, the generic engine at 1 GiB.
export OUT=${OUT:-out}  # where the results go (relative to the repository root)
TAG=${1:-r06}
mkdir -p $OUT
timeout 900 python -m pytest tests -m gpu -q -x 2>&1 | tail -4 > $OUT/${TAG}_pytest_gpu.log; cat $OUT/${TAG}_pytest_gpu.log
timeout 300 python -m pytest tests/test_reference_package.py tests/test_real_vocab.py -m gpu -v 2>&1 | grep -v "^$" | tail -45 > $OUT/${TAG}_reference_package_over_shim.txt; tail -3 $OUT/${TAG}_reference_package_over_shim.txt
timeout 100 python __graft_entry__.py smoke 2>&1 | tail -1
timeout 600 bash tools/gpu_prof.sh 1024 $TAG > $OUT/${TAG}_prof.log 2>&1; tail -2 $OUT/${TAG}_prof.log | cut -c1-200
timeout 600 bash tools/gpu_pmc.sh > $OUT/${TAG}_pmc.log 2>&1; tail -3 $OUT/${TAG}_pmc.log
timeout 600 bash tools/gpu_phases.sh $TAG > $OUT/${TAG}_front_phases.csv 2> $OUT/${TAG}_front_phases.err; cat $OUT/${TAG}_front_phases.csv
NOPAR=1 timeout 300 bash tools/gpu_ab.sh "timing|timing|" > $OUT/${TAG}_front_cycles.log 2>&1; python - <<PY > $OUT/${TAG}_front_cycles.txt
import json
for l in open("gpurun_out/ab/exp.jsonl"):
    j = json.loads(l); print(j["tag"], "front ms", j["kernels_ms"]["tk_k_front"], "cycles per tile and phase", j.get("cycles_per_tile"))
PY
cat $OUT/${TAG}_front_cycles.txt
timeout 100 tools/ubench/pcie_rates > $OUT/${TAG}_pcie_link.txt 2>&1; cat $OUT/${TAG}_pcie_link.txt
timeout 500 python bench.py --full > $OUT/${TAG}_bench_1gpu.json 2> $OUT/${TAG}_bench.err; cut -c1-400 $OUT/${TAG}_bench_1gpu.json; tail -2 $OUT/${TAG}_bench.err
timeout 400 python tools/bench_configs.py > $OUT/${TAG}_configs.jsonl 2> $OUT/${TAG}_configs.err; cut -c1-200 $OUT/${TAG}_configs.jsonl
timeout 300 python tools/small_call.py > $OUT/${TAG}_small_calls.txt 2>&1; tail -4 $OUT/${TAG}_small_calls.txt
timeout 120 python tools/mid_corpus.py > $OUT/${TAG}_mid_calls_corpus.txt 2>&1; tail -4 $OUT/${TAG}_mid_calls_corpus.txt
timeout 300 python tools/stress_repeats.py o200k_shaped > $OUT/${TAG}_long_runs.txt 2>&1; tail -5 $OUT/${TAG}_long_runs.txt
timeout 400 python bench.py --full --generic-engine --steps 3 --warmup 1 --no-host-path > $OUT/${TAG}_bench_generic_engine.json 2> $OUT/${TAG}_bench_generic_engine.err; cut -c1-300 $OUT/${TAG}_bench_generic_engine.json
