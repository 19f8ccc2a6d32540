#!/bin/bash
# A/B of library builds on the driver's command (bench.py --gpus 1 --steps 20 --warmup 5), the
# builds interleaved (a b c a b c ...) so that drift of the machine falls on all of them alike.
# A build is a TWOSD_LIB variant (sqlp_amd/libtwosd_hip_<variant>.so); "default" is libtwosd_hip.so.
# Every run dumps its outputs (--dump-outputs) for the byte comparison of tools/ab_lp_summary.py.
# Usage (repo root, GPU box): bash tools/ab_lp_builds.sh <session dir> <reps> <variant> [<variant> ...]
# Writes <session dir>/bench_<variant>_<rep>.json and dump_<variant>_<rep>/; stops at the first failure.
set -u
OUT=$1; REPS=$2; shift 2
mkdir -p $OUT
for rep in $(seq 1 $REPS); do
  for v in "$@"; do
    lib=$v; [ "$v" = default ] && lib=""
    TWOSD_LIB=$lib timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs $OUT/dump_${v}_$rep \
        > $OUT/bench_${v}_$rep.json 2> $OUT/bench_${v}_$rep.err
    rc=$?
    if [ $rc -ne 0 ]; then echo "[$v] run $rep rc=$rc"; tail -5 $OUT/bench_${v}_$rep.err; exit $rc; fi
    python3 - $OUT/bench_${v}_$rep.json "$v" $rep <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
ph = d["phases_ms_per_step"]
print(f"[{sys.argv[2]} #{sys.argv[3]}] lp {ph['lp_kernel']:.2f} ms, step {d['ms_per_step']:.2f} ms, piv {d['lp_pivots_mean']:.4f}", flush=True)
PY
  done
done
