#!/bin/bash
# usage (on the GPU box): [PROF_OUT=<dir>] tools/prof_quick.sh <tag>   -> <dir>/prof_<tag>/ (default dir: prof_out) + family summary on stdout
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
O="${PROF_OUT:-prof_out}/prof_$1"
rm -rf "$O" && mkdir -p "$(dirname "$O")" || exit 1
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$O" -o $1 --output-format csv -- python3 bench.py --full --steps 3 --warmup 2 --no-cpu-baseline > "$O.json" 2> "$O.err" || exit 1
python3 tools/prof_summary.py "$O" | sed -n '/last full step/,$p' | head -${2:-16}
