#!/bin/bash
# Measurements of evolve_pareto beside evolve at J6M6E2 x 4096, P = 32 (tools/measure_pareto.py explains) ->
# $MTFJSP_TOOL_OUT/pareto.json (default tool_out/), to be copied to profiles/pareto.json.  The kernel-trace runs stand alone (no
# counters); every GPU step has its own time limit and a failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" &&
timeout -k 10 120 python3 tools/measure_pareto.py --mode chain > "$MTFJSP_TOOL_OUT/pareto_chain.log" 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/pareto_trace_pareto" -- python3 tools/measure_pareto.py --mode trace --what pareto > "$MTFJSP_TOOL_OUT/pareto_trace_pareto.log" 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/pareto_trace_evolve" -- python3 tools/measure_pareto.py --mode trace --what evolve > "$MTFJSP_TOOL_OUT/pareto_trace_evolve.log" 2>&1 &&
timeout -k 10 400 python3 tools/measure_pareto.py --mode wall > "$MTFJSP_TOOL_OUT/pareto_wall.log" 2>&1 &&
python3 tools/measure_pareto.py --mode reduce
