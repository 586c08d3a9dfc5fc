#!/bin/bash
# Round 5, last GPU call: the GPU suite and the round's profiles on the final code (kernel stats, HBM traffic, SQ counters, bench line, configs, the generic engine at 1 GiB)
export OUT=${OUT:-out}  # where the results go (relative to the repository root)
TAG=r05
mkdir -p $OUT
timeout 700 python -m pytest tests -m gpu -q -x 2>&1 | tail -4 > $OUT/${TAG}_pytest_gpu.log; cat $OUT/${TAG}_pytest_gpu.log
timeout 100 python __graft_entry__.py smoke 2>&1 | tail -1
timeout 600 bash tools/gpu_prof.sh 1024 $TAG > $OUT/${TAG}_prof.log 2>&1; tail -2 $OUT/${TAG}_prof.log | cut -c1-200
timeout 600 bash tools/gpu_pmc.sh > $OUT/${TAG}_pmc.log 2>&1; tail -3 $OUT/${TAG}_pmc.log
timeout 400 python bench.py --full > $OUT/${TAG}_bench_1gpu.json 2> $OUT/${TAG}_bench.err; cut -c1-400 $OUT/${TAG}_bench_1gpu.json
timeout 300 python tools/bench_configs.py > $OUT/${TAG}_configs.jsonl 2> $OUT/${TAG}_configs.err; cut -c1-200 $OUT/${TAG}_configs.jsonl
timeout 400 python bench.py --full --generic-engine --steps 3 --warmup 1 --no-host-path > $OUT/${TAG}_bench_generic_engine.json 2> $OUT/${TAG}_bench_generic_engine.err; cut -c1-300 $OUT/${TAG}_bench_generic_engine.json
