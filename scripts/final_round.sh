#!/bin/bash
# Round-6 final evidence on the GPU box: profiles (scripts/profile_round.sh), then the GPU suite, smoke and the `--full` bench line
O=${1:?usage: scripts/final_round.sh OUTDIR}; mkdir -p "$O"
bash scripts/profile_round.sh > "$O/r6_profile_round.log" 2>&1
bash scripts/evidence_run.sh "$O"
