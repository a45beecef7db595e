#!/bin/bash
# Development tool (GPU box): the driver's three steps - suite, smoke, bench - then the profile passes behind profiles/round6_*
# and the SURVEY 8(d) sweep, on one box.  usage: gpurun -- 'bash tools/validate.sh [tag] [steps...]'
#   steps (default: all): tests smoke bench (with --full) profiles suite; the logs go to $OUT (default: validate_logs/)
cd "${GRAFT_REPO_ROOT:-.}"
OUT=${OUT:-validate_logs}; mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
TAG=${1:-r6}; shift
STEPS=${*:-tests smoke bench profiles suite}
for s in $STEPS; do
  case $s in
    tests)    ( time timeout 1500 python -m pytest tests -x -q -m gpu --durations=15 ) > "$OUT/${TAG}_tests.log" 2>&1; tail -22 "$OUT/${TAG}_tests.log" ;;
    smoke)    python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/${TAG}_smoke.log" 2>&1; tail -2 "$OUT/${TAG}_smoke.log" ;;
    bench)    ( time timeout 900 python bench.py --steps 20 --warmup 5 --full ) > "$OUT/${TAG}_bench.log" 2> "$OUT/${TAG}_bench.err"
              cp bench_last.json "$OUT/${TAG}_bench_last.json"; tail -3 "$OUT/${TAG}_bench.err"; cut -c1-1500 "$OUT/${TAG}_bench.log" ;;
    profiles) bash tools/round6_profiles.sh > "$OUT/${TAG}_profiles.log" 2>&1; tail -12 "$OUT/${TAG}_profiles.log" ;;
    suite)    timeout 1200 python tools/suite.py > "$OUT/${TAG}_suite.log" 2>&1; tail -3 "$OUT/${TAG}_suite.log" ;;
  esac
done
