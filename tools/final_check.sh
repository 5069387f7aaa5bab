#!/bin/bash
# End-of-change check on an MI355X: the GPU suite, smoke(), and the full bench line with its wall time.
# Usage: tools/final_check.sh OUTDIR   (logs: OUTDIR/final_suite.log, OUTDIR/final_bench.log)
mkdir -p "${1:?usage: tools/final_check.sh OUTDIR}"
O=$(cd "$1" && pwd)
cd "$(dirname "$0")/.."
( time timeout 2400 python -m pytest tests -x -q -m gpu ) > $O/final_suite.log 2>&1; tail -6 $O/final_suite.log | cut -c1-200
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
( time python bench.py --full ) > $O/final_bench.log 2>&1; grep -o '"value": [0-9.]*\|"ms_per_step": [0-9.]*\|"frac": [0-9.]*\|"traffic_source": "[^"]*"\|real.*' $O/final_bench.log | head -12
