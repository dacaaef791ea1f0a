#!/bin/bash
# Measurements of local search on plans at J6M6E2 x 1024, K = 32, 32 rounds (tools/profile_plan_search.py explains) ->
# $MTFJSP_TOOL_OUT/plan_search.json (default tool_out/), to be copied to profiles/plan_search.json.  The kernel-trace run stands
# alone (no counters); every GPU step has its own time limit and a failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" &&
timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/plan_search_trace" -- python3 tools/profile_plan_search.py --mode trace > "$MTFJSP_TOOL_OUT/plan_search_trace.log" 2>&1 &&
timeout -k 10 300 python3 tools/profile_plan_search.py --mode wall > "$MTFJSP_TOOL_OUT/plan_search_wall.log" 2>&1 &&
timeout -k 10 300 python3 tools/profile_plan_search.py --mode quality > "$MTFJSP_TOOL_OUT/plan_search_quality.log" 2>&1 &&
python3 tools/profile_plan_search.py --mode reduce
