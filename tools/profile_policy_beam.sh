#!/bin/bash
# Measurements of the policy-guided beam search at J6M6E2, N*W = 2048 slots at W = 8 (tools/profile_policy_beam.py explains)
# -> $MTFJSP_TOOL_OUT/policy_beam.json (default tool_out/), to be copied to profiles/policy_beam.json.  The kernel-trace run stands
# alone (no counters); every GPU step has its own time limit and a failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" &&
timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/policy_beam_trace" -- python3 tools/profile_policy_beam.py --mode trace > "$MTFJSP_TOOL_OUT/policy_beam_trace.log" 2>&1 &&
timeout -k 10 240 python3 tools/profile_policy_beam.py --mode wall > "$MTFJSP_TOOL_OUT/policy_beam_wall.log" 2>&1 &&
timeout -k 10 300 python3 examples/policy_beam.py --json "$MTFJSP_TOOL_OUT/policy_beam_quality.json" > "$MTFJSP_TOOL_OUT/policy_beam_example.log" 2>&1 &&
timeout -k 10 300 python3 -m pytest -q -s -p no:cacheprovider tests/test_policy_beam_gpu.py > "$MTFJSP_TOOL_OUT/policy_beam_replay.log" 2>&1 &&
python3 tools/profile_policy_beam.py --mode reduce
