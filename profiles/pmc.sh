#!/bin/bash
# Collects rocprofv3 PMC counters for the benchmark kernels in separate passes (kernel-trace only, no other trace
# domains), as /opt/skills/guides/MI355X_MICROARCH.md section HBM prescribes.  Usage (on the GPU box, from the
# repository root):  bash profiles/pmc.sh <out_dir> [bench args]
# Every pass runs under a time limit, and the first pass that fails ends the script: nothing more starts on the card after it.
set -u
OUT=$(realpath -m "$1"); shift
mkdir -p "$OUT"
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
ARGS="--steps 3 --warmup 1 --no-cpu-baseline --no-secondary $*"
run() { # name, counters
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $2 --output-format csv -d "$OUT/$1" -- python3 "$ROOT/bench.py" $ARGS > "$OUT/$1.log" 2>&1
  local rc=$?
  echo "$1 rc=$rc"
  if [ $rc != 0 ]; then tail -20 "$OUT/$1.log" >&2; exit $rc; fi
}
run fetch "FETCH_SIZE"
run write "WRITE_SIZE"
run sq1 "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU"
run sq2 "SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"
