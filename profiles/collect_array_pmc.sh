#!/bin/bash
# HBM bytes of the split-step kernels: two counter-only rocprofv3 passes (no tracing in the same run), each under its own
# time limit; the second starts only if the first ended well.
#   bash profiles/collect_array_pmc.sh [OUT.txt]     (default: profiles/array_strategies_pmc.txt)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$ROOT/profiles/array_strategies_pmc.txt}
WORK=$(mktemp -d)
cd "$WORK" &&
timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$WORK/fetch" -o fetch -- python3 "$ROOT/profiles/array_strategies_pmc.py" > "$WORK/fetch.log" 2>&1 &&
timeout -k 10 240 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$WORK/write" -o write -- python3 "$ROOT/profiles/array_strategies_pmc.py" > "$WORK/write.log" 2>&1 &&
python3 "$ROOT/profiles/array_strategies_pmc.py" --summarise "$WORK" "$OUT"
rc=$?
[ $rc -ne 0 ] && tail -5 "$WORK"/*.log
exit $rc
