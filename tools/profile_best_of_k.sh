#!/bin/bash
# Measurements of best-of-K evaluation at J6M6E2 x 1024 (tools/profile_best_of_k.py explains) -> $MTFJSP_TOOL_OUT/best_of_k.json
# (default tool_out/), to be copied to profiles/best_of_k.json.  The kernel-trace run stands alone (no counters); every GPU step has
# its own time limit and a failing step ends the script.  A wall-time run of validate_cost_batched against another build of the
# library (the parent commit's: run `profile_best_of_k.py --mode wall --only-validate --wall-json $MTFJSP_TOOL_OUT/best_of_k_wall_parent.json`
# from that checkout first) is folded in when its file is there.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" &&
timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/best_of_k_trace" -- python3 tools/profile_best_of_k.py --mode trace > "$MTFJSP_TOOL_OUT/best_of_k_trace.log" 2>&1 &&
timeout -k 10 300 python3 tools/profile_best_of_k.py --mode wall > "$MTFJSP_TOOL_OUT/best_of_k_wall.log" 2>&1 &&
timeout -k 10 300 python3 tools/profile_best_of_k.py --mode quality > "$MTFJSP_TOOL_OUT/best_of_k_quality.log" 2>&1 &&
python3 tools/profile_best_of_k.py --mode reduce
