#!/bin/bash
# Measurements of local search with critical-path moves at J6M6E2 x 4096, K = 16 (tools/profile_critical_search.py explains) ->
# $MTFJSP_TOOL_OUT/critical_search.json (default tool_out/), to be copied to profiles/critical_search.json.  Every profiled run stands
# alone (kernel trace, no counters); every GPU step has its own time limit and a failing step ends the script.
# PARENT_TREE: another built checkout of this repository (the parent commit) for the A/B of the old instantiation; without it the
# A/B is recorded as unmeasured.
set -o pipefail
cd "$(dirname "$0")/.." && export MTFJSP_TOOL_OUT=${MTFJSP_TOOL_OUT:-tool_out} TMPDIR=${TMPDIR:-/tmp} && mkdir -p "$MTFJSP_TOOL_OUT" || exit 1
O=$MTFJSP_TOOL_OUT
P="python3 tools/profile_critical_search.py --out-dir $O"
prof() { local d=$1; shift; timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/$d" -- "$@" > "$O/$d.log" 2>&1; }
prof critical_trace $P --mode trace || exit 1
if [ -n "$PARENT_TREE" ]; then
    for i in 1 2 3; do
        prof critical_ab_parent_$i $P --mode ab --tree "$PARENT_TREE" && prof critical_ab_this_$i $P --mode ab || exit 1
    done
fi
timeout -k 10 300 $P --mode wall > "$O/critical_wall.log" 2>&1 &&
timeout -k 10 400 $P --mode quality > "$O/critical_quality.log" 2>&1 &&
$P --mode reduce
