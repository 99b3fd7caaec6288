#!/bin/bash
# Round-end measurement: the GPU tests, the full bench line, then the round profile.
# Logs go to $LOGS (default: logs/ in the repository root, git-ignored).
set -u
cd "$(dirname "$0")/.."
LOGS=${LOGS:-logs}
mkdir -p "$LOGS"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$LOGS/tests_final.log" 2>&1 || { echo "tests rc=$?"; tail -20 "$LOGS/tests_final.log"; exit 1; }
tail -1 "$LOGS/tests_final.log"
timeout -k 10 900 python -u bench.py --full > "$LOGS/bench_final.log" 2>&1 || { echo "bench rc=$?"; tail -20 "$LOGS/bench_final.log"; exit 1; }
tail -1 "$LOGS/bench_final.log" | cut -c1-300
timeout -k 10 1100 bash scripts/profile_round.sh ${ROUND:-r05} > "$LOGS/prof_${ROUND:-r05}.log" 2>&1 || { echo "prof rc=$?"; tail -20 "$LOGS/prof_${ROUND:-r05}.log"; exit 1; }
tail -5 "$LOGS/prof_${ROUND:-r05}.log"
