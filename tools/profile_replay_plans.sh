#!/bin/bash
# Measurements of the plan replay in one launch (tools/profile_replay_plans.py explains) -> $MTFJSP_TOOL_OUT/replay_plans.json (default
# tool_out/), to be copied to profiles/replay_plans.json.  MTFJSP_PARENT_ROOT: a built checkout of the parent commit; its step-launch
# form is then timed before and after this tree's two forms, on the same box.  The kernel-trace run stands alone (no counters); every
# GPU step has its own time limit and a failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" &&
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$MTFJSP_TOOL_OUT/replay_plans_trace" -- python3 tools/profile_replay_plans.py --mode trace > "$MTFJSP_TOOL_OUT/replay_plans_trace.log" 2>&1 &&
{ [ -z "$MTFJSP_PARENT_ROOT" ] || timeout -k 10 300 python3 tools/profile_replay_plans.py --mode wall --root "$MTFJSP_PARENT_ROOT" --replay parent --tag wall_parent_before > "$MTFJSP_TOOL_OUT/replay_plans_wall_parent_before.log" 2>&1; } &&
timeout -k 10 300 python3 tools/profile_replay_plans.py --mode wall --tag wall_this_tree > "$MTFJSP_TOOL_OUT/replay_plans_wall_this_tree.log" 2>&1 &&
{ [ -z "$MTFJSP_PARENT_ROOT" ] || timeout -k 10 300 python3 tools/profile_replay_plans.py --mode wall --root "$MTFJSP_PARENT_ROOT" --replay parent --tag wall_parent_after > "$MTFJSP_TOOL_OUT/replay_plans_wall_parent_after.log" 2>&1; } &&
python3 tools/profile_replay_plans.py --mode reduce
