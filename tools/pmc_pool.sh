#!/bin/bash
# PMC passes over the vote pool (one rocprofv3 --pmc run per counter group: <= 8 SQ counters,
# FETCH_SIZE and WRITE_SIZE alone) on tools/pool_probe.py's pre-published mode (prog 2: six
# 4,096-vote batches published before the grids start, so the counters hold no idle wait),
# then tools/pmc_pool_summary.py. TAG=r05x bash tools/pmc_pool.sh   (GPU box, repo root)
# Passes c and d are the instruction-fetch and instruction-cache counters (summarised by
# tools/pmc_pool_summary.py TAG icache NAME). PASSES="c d" runs only those; LIB=file.so (under
# consensus_overlord_amd/) profiles another build of the library.
# rocprofv3 serialises dispatches: every pass sees the pool alone on the device, without the
# final-stream kernels that share its CUs in a pipelined run.
set -euo pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R=$(pwd)
OUT=$R/gpurun_out/${TAG:-pmc}/pmcpool
mkdir -p "$OUT"
export TMPDIR=/tmp
[ -n "${LIB:-}" ] && export OVH_LIBPATH=$R/consensus_overlord_amd/$LIB
cd /tmp
P="python3 $R/tools/pool_probe.py 4096 6 2 1"
want() { case " ${PASSES:-a b c d fetch write kt} " in *" $1 "*) return 0 ;; esac; return 1; }
pmc() {  # pass name, counters...
  local n=$1
  shift
  timeout -s KILL 120 rocprofv3 --pmc "$@" -d "$OUT/$n" -o "$n" --output-format csv -- $P > "$OUT/$n.log" 2>&1
}
if want a; then
  pmc a SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY
fi
if want b; then
  pmc b SQ_WAVES SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_INSTS_VALU_INT64 SQ_INSTS_VALU_INT32 SQ_ACTIVE_INST_LDS \
    SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE
fi
if want c; then
  pmc c SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_IFETCH SQ_IFETCH_LEVEL SQ_INSTS_BRANCH SQ_BUSY_CYCLES
fi
if want d; then
  pmc d SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE SQC_ICACHE_BUSY_CYCLES \
    SQC_ICACHE_INPUT_VALID_READYB SQC_TC_INST_REQ
fi
if want fetch; then pmc fetch FETCH_SIZE; fi
if want write; then pmc write WRITE_SIZE; fi
if want kt; then
  timeout -s KILL 120 rocprofv3 --kernel-trace --stats -d "$OUT/kt" -o kt --output-format csv -- $P > "$OUT/kt.log" 2>&1
fi
echo done > "$OUT/ok"
