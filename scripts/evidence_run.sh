#!/bin/bash
# Round-6 evidence run on the GPU box: the whole GPU suite, smoke, the `--full` bench line (N = 1), written to OUTDIR
O=${1:?usage: scripts/evidence_run.sh OUTDIR}; mkdir -p "$O"
python -m pytest tests -m gpu -q 2>&1 | tail -8 > "$O/r6_pytest_gpu_tail.txt"
python -c "import __graft_entry__ as g; g.smoke()" > "$O/r6_smoke.txt" 2>&1
( time python bench.py --full --steps 20 --warmup 5 > "$O/r6_bench_n1.json" 2> "$O/r6_bench_n1.err" ) 2> "$O/r6_bench_time.txt"
cat "$O/r6_pytest_gpu_tail.txt" "$O/r6_smoke.txt" "$O/r6_bench_time.txt"
