#!/bin/bash
# rocprofv3 kernel trace of the 8,192-stream streaming leg: per-tick kernel/gap timeline + scorer histogram
R="${GRAFT_REPO_ROOT:-/root/repo}"
OUT="${EWK_OUT:-$R/out}"; mkdir -p "$OUT"   # logs and profiler output
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/tprof -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 \
   --no-cpu-baseline --fixed-len 0 --confirm-batch 0 --big-streams 0 --max-streams 0 > $OUT/tprof.log 2>&1 || exit $?
python $R/scripts/tick_hist.py $OUT/tprof > $OUT/tick_hist.txt && echo '-- timed ticks (no event records):' >> $OUT/tick_hist.txt && python $R/scripts/tick_timeline.py $OUT/tprof 12 420 >> $OUT/tick_hist.txt && echo '-- instrumented ticks (event records around each kernel):' >> $OUT/tick_hist.txt && python $R/scripts/tick_timeline.py $OUT/tprof 6 >> $OUT/tick_hist.txt
rc=$?
find $OUT/tprof -name "*kernel_trace.csv" -delete
cat $OUT/tick_hist.txt
exit $rc
