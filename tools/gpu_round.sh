#!/bin/bash
# One GPU-box session: GPU parity tests, the bench line, a rocprofv3 kernel-trace/stats run of the same bench
# command, and two separate PMC passes (FETCH_SIZE, WRITE_SIZE) of tools/pmc_forward.py.  Every GPU step has its
# own time limit; after a fault / abort / timeout nothing further runs on the GPU.
#   bash tools/gpu_round.sh [tests|bench|prof|pmc|optable ...]   (default: tests bench prof pmc)
# BENCH_ARGS / PMC_ARGS / OPT_ARGS: extra arguments of the prof-step bench, tools/pmc_forward.py, tools/op_table.py
# OUT: the directory (relative to the repository) the logs and results go to (default bench_out)
cd "$(dirname "$0")/.." || exit 1
ROOT=$PWD
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp YM_TUNE_DIR="$ROOT/$OUT/tune"
steps=("$@"); [ ${#steps[@]} -eq 0 ] && steps=(tests bench prof pmc)
fatal() { local rc=$1; [ "$rc" -eq 124 ] || [ "$rc" -eq 137 ] || [ "$rc" -eq 134 ] || [ "$rc" -eq 139 ] || [ "$rc" -gt 128 ]; }
for s in "${steps[@]}"; do
  echo "[gpu_round] step $s $(date +%T)"
  case $s in
    tests) timeout -k 10 900 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread > "$OUT/gt.log" 2>&1; rc=$?
           tail -15 "$OUT/gt.log" ;;
    qtests) timeout -k 10 600 python -u -m pytest tests/test_gpu_quant.py -v -p no:cacheprovider --timeout 240 --timeout-method thread > "$OUT/qt.log" 2>&1; rc=$?
           tail -25 "$OUT/qt.log" ;;
    bench_i8) timeout -k 10 500 python bench.py --full --dtype i8 > "$OUT/bench_i8.json" 2> "$OUT/bench_i8.err"; rc=$?
           cat "$OUT/bench_i8.json"; tail -3 "$OUT/bench_i8.err" ;;
    bench) timeout -k 10 400 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; rc=$?
           cat "$OUT/bench.json" ;;
    bench_s) timeout -k 10 400 python bench.py --full --model s > "$OUT/bench_s.json" 2> "$OUT/bench_s.err"; rc=$?
           cat "$OUT/bench_s.json" ;;
    prof)  cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv \
             -d "$ROOT/$OUT/prof_bench" -o run -- python3 "$ROOT/bench.py" --full --steps 50 \
             --warmup 10 --no-cpu --no-f16 $BENCH_ARGS > "$ROOT/$OUT/prof_bench.log" 2>&1; rc=$?; cd "$ROOT" ;;
    pmc)   cd /tmp && timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv \
             -d "$ROOT/$OUT/pmc_fetch" -o run -- python3 "$ROOT/tools/pmc_forward.py" $PMC_ARGS \
             > "$ROOT/$OUT/pmc_fetch.log" 2>&1; rc=$?
           if [ $rc -eq 0 ]; then timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv \
             -d "$ROOT/$OUT/pmc_write" -o run -- python3 "$ROOT/tools/pmc_forward.py" $PMC_ARGS \
             > "$ROOT/$OUT/pmc_write.log" 2>&1; rc=$?; fi
           cd "$ROOT" ;;
    optable) timeout -k 10 300 python -u tools/op_table.py $OPT_ARGS > "$OUT/op_table.txt" 2>&1; rc=$?
           tail -3 "$OUT/op_table.txt" ;;
    *) echo "unknown step $s"; rc=2 ;;
  esac
  echo "[gpu_round] step $s rc=$rc $(date +%T)"
  if fatal $rc; then echo "[gpu_round] fatal rc=$rc in $s: stopping"; exit $rc; fi
  if [ "$rc" -ne 0 ]; then any_fail=$rc; fi
done
exit ${any_fail:-0}
