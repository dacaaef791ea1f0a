#!/bin/bash
# Measurements of evolve beside local_search at J6M6E2 x 4096, P = K = 16 (tools/measure_evolve.py explains) ->
# $MTFJSP_TOOL_OUT/evolve.json (default tool_out/), to be copied to profiles/evolve.json.  The kernel-trace runs stand alone (no
# counters); every GPU step has its own time limit and a failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" &&
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/evolve_trace_evolve" -- python3 tools/measure_evolve.py --mode trace --what evolve > "$MTFJSP_TOOL_OUT/evolve_trace_evolve.log" 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/evolve_trace_ls" -- python3 tools/measure_evolve.py --mode trace --what ls > "$MTFJSP_TOOL_OUT/evolve_trace_ls.log" 2>&1 &&
timeout -k 10 300 python3 tools/measure_evolve.py --mode wall > "$MTFJSP_TOOL_OUT/evolve_wall.log" 2>&1 &&
timeout -k 10 300 python3 tools/measure_evolve.py --mode quality > "$MTFJSP_TOOL_OUT/evolve_quality.log" 2>&1 &&
python3 tools/measure_evolve.py --mode reduce
