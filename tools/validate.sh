#!/bin/bash
# End-of-round validation on the GPU box (from the repo root): the GPU test suite, smoke(), the
# default bench line, the stack, synthetic and partitioned bench lines (each with --full: roofline,
# variants, CPU baselines). Usage: tools/validate.sh [OUTDIR]   (default out/final, git-ignored)
set -o pipefail
OUT=${1:-out/final}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests -m gpu > $OUT/t.log 2>&1 &&
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1 &&
timeout -k 10 400 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err &&
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_20.json 2> $OUT/bench_20.err &&
timeout -k 10 300 python bench.py --full --workload stack > $OUT/bench_stack.json 2> $OUT/bench_stack.err &&
timeout -k 10 300 python bench.py --full --workload synthetic > $OUT/bench_synth.json 2> $OUT/bench_synth.err &&
timeout -k 10 300 python bench.py --full --partitioned --no-cpu-baseline > $OUT/bench_part.json 2> $OUT/bench_part.err
rc=$?; tail -3 $OUT/t.log; cat $OUT/smoke.log 2>/dev/null | tail -1
for f in $OUT/bench*.json; do echo "$f"; tail -1 "$f" | cut -c1-300; done
exit $rc
