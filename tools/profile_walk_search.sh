#!/bin/bash
# Measurements of walk_search beside local_search at J6M6E2 x 4096, K = 16 (tools/profile_walk_search.py explains) ->
# $MTFJSP_TOOL_OUT/walk_search.json (default tool_out/), to be copied to profiles/walk_search.json.  The profiled run stands alone
# (kernel trace, no counters); every GPU step has its own time limit and a failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" || exit 1
O=$MTFJSP_TOOL_OUT
P="python3 tools/profile_walk_search.py --out-dir $O"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/walk_trace" -- $P --mode trace > "$O/walk_trace.log" 2>&1 &&
timeout -k 10 240 $P --mode wall > "$O/walk_wall.log" 2>&1 &&
timeout -k 10 400 $P --mode quality > "$O/walk_quality.log" 2>&1 &&
$P --mode reduce
