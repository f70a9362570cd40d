#!/bin/bash
# One session on the GPU: parity tests, smoke, the whole bench (--full), rocprofv3 kernel trace.  Everything lands in $O/.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
O=${BRC_OUT_DIR:-bench_out}; mkdir -p $O
export TMPDIR=/tmp
echo "== nproc $(nproc); $(rocminfo 2>/dev/null | grep -m1 gfx9 || true)" | tee $O/session.log
( time timeout 900 python -m pytest tests -q -m gpu ) > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?" | tee -a $O/session.log
tail -5 $O/pytest_gpu.log | tee -a $O/session.log
( time timeout 300 python __graft_entry__.py smoke ) > $O/smoke.log 2>&1; echo "smoke rc=$?" | tee -a $O/session.log
tail -3 $O/smoke.log | tee -a $O/session.log
( time timeout 900 python bench.py --full --steps ${BENCH_STEPS:-10} --warmup 2 ${BENCH_ARGS:-} ) > $O/bench.log 2>&1; echo "bench rc=$?" | tee -a $O/session.log
tail -4 $O/bench.log | tee -a $O/session.log
if [ "${DO_PROF:-1}" = "1" ]; then
  rm -rf $O/prof
  ( cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OLDPWD/$O/prof" -o trace -- python "$OLDPWD/bench.py" --steps 5 --warmup 1 --cpu-sample-mbp 0 ${BENCH_ARGS:-} ) > $O/rocprof.log 2>&1; echo "rocprof rc=$?" | tee -a $O/session.log
  find $O/prof -name "*stats*" | head | tee -a $O/session.log
  f=$(find $O/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -20 "$f" | tee -a $O/session.log
  # keep the merge small: drop the big per-dispatch trace, keep stats
  find $O/prof -name "*kernel_trace.csv" -size +20M -delete
fi
