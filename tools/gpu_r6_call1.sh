#!/bin/bash
# Round 6, first GPU call: the GPU suite on the round's first commit (new tests included), the N > 1 dry run with the two-phase gather probe,
# the baseline bench line before any kernel change, N1g.
export OUT=${OUT:-out}  # where the results go (relative to the repository root)
mkdir -p $OUT
timeout 900 python -m pytest tests -m gpu -q -x 2>&1 | tail -6 > $OUT/r06a_pytest_gpu.log; cat $OUT/r06a_pytest_gpu.log
timeout 300 python -m pytest tests/test_reference_package.py tests/test_real_vocab.py -m gpu -v 2>&1 | tail -40 > $OUT/r06a_refpkg.log; tail -25 $OUT/r06a_refpkg.log
timeout 400 bash tools/gpu_bench_n2_dry.sh 256 > $OUT/r06a_bench_n2_dry.txt 2>&1; tail -c 1500 $OUT/r06a_bench_n2_dry.txt
timeout 500 python bench.py --full > $OUT/r06a_bench_1gpu.json 2> $OUT/r06a_bench.err; cut -c1-600 $OUT/r06a_bench_1gpu.json; tail -3 $OUT/r06a_bench.err
