#!/bin/bash
# Regenerates the artefacts kept under profiles/ for one round, on an MI355X: tools/profile_round.sh TAG OUTDIR
# Output: OUTDIR/{bench.json,bench_200.json,clocks.txt,event_table.json,kernel_stats_{two,single}.csv,timeline_*,gaps_*.txt}
# (tools/collect_profiles.py TAG copies them into profiles/ from the scratch directory it reads)
TAG=${1:?usage: tools/profile_round.sh TAG OUTDIR}
mkdir -p "${2:?usage: tools/profile_round.sh TAG OUTDIR}"
O=$(cd "$2" && pwd)
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
cd $R
# the clocks the chip holds while the step runs: every 100-ms sample of the timed loop + a rocm-smi snapshot
python bench.py --steps 200 --warmup 10 --clock-log $O/clocks.txt > $O/bench_200.json 2> /dev/null
( echo "# rocm-smi right after the loop:"; rocm-smi --showclocks --showpower 2>/dev/null | grep -E "GPU\[|sclk|Power" ) >> $O/clocks.txt
python bench.py --full --steps 50 --warmup 10 --kernel-table $O/event_table.json > $O/bench.json 2> $O/bench.err
cd /tmp
rocprofv3 --kernel-trace --stats -d $O/two -o r -- python3 $R/bench.py --steps 12 --warmup 4 > $O/two.log 2>&1
FRHIP_SINGLE_STREAM=1 rocprofv3 --kernel-trace --stats -d $O/single -o r -- python3 $R/bench.py --steps 12 --warmup 4 > $O/single.log 2>&1
cd $R
for m in two single; do db=$(find $O/$m -name "*.db" | head -1); python tools/trace_gaps.py $db --csv $O/kernel_stats_$m.csv --timeline $O/timeline_$m.txt > $O/gaps_$m.txt 2>&1; done
find $O -name "*.db" -delete
tail -3 $O/bench.json | cut -c1-600; head -8 $O/gaps_two.txt; head -8 $O/gaps_single.txt
