#!/bin/bash
# Measurements of the beam search at J6M6E2 x 1024, W = 8 (tools/profile_beam.py explains) -> $MTFJSP_TOOL_OUT/beam_baselines.json
# (default tool_out/), to be copied to profiles/beam_baselines.json.  The kernel-trace run stands alone (no counters); every GPU
# step has its own time limit and a failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" &&
timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/beam_trace" -- python3 tools/profile_beam.py --mode trace > "$MTFJSP_TOOL_OUT/beam_trace.log" 2>&1 &&
timeout -k 10 240 python3 tools/profile_beam.py --mode wall > "$MTFJSP_TOOL_OUT/beam_wall.log" 2>&1 &&
timeout -k 10 300 python3 tools/profile_beam.py --mode quality > "$MTFJSP_TOOL_OUT/beam_quality.log" 2>&1 &&
python3 tools/profile_beam.py --mode reduce
