#!/bin/bash
# Measurements of the fork and the look-ahead rules at J6M6E2 x 1024 (tools/profile_lookahead.py explains) -> $MTFJSP_TOOL_OUT/lookahead_baselines.json
# (default tool_out/), to be copied to profiles/lookahead_baselines.json.  The kernel-trace run stands alone (no counters); every GPU
# step has its own time limit and a failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" &&
timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/lookahead_trace" -- python3 tools/profile_lookahead.py --mode trace > "$MTFJSP_TOOL_OUT/lookahead_trace.log" 2>&1 &&
timeout -k 10 240 python3 tools/profile_lookahead.py --mode wall > "$MTFJSP_TOOL_OUT/lookahead_wall.log" 2>&1 &&
python3 tools/profile_lookahead.py --mode reduce
