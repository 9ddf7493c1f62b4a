#!/bin/bash
# tools/acq_quick.sh [frames...] -- the FFT-acquire GPU tests, then one short bench line per frame size with the phase clocks
export JSDR_KNOBS=1 JSDR_BENCH_ALLOW_KNOBS=1 JSDR_BENCH_LIVE_TRAFFIC=0  # the library listens to its tuning knobs only with JSDR_KNOBS=1; bench.py measures with them only when told
O=${JSDR_OUT:-bench_out}; mkdir -p $O; export TMPDIR=/tmp  # logs go to $JSDR_OUT (default bench_out/)
timeout -k 10 800 python -m pytest tests/test_gpu_bpsk.py tests/test_gpu_fixtures.py -m gpu -q -x -p no:cacheprovider --timeout 600 -k "fft or acq or mixed or 9600 or 4800 or 19200" > $O/t_acq.log 2>&1
tail -3 $O/t_acq.log
for F in ${*:-9600}; do
  JSDR_FFT_PHASECLK=1 timeout -k 10 300 python bench.py --workload bpsk --fft-acquire --bpsk-frame $F --streams 1024 --full --no-cpu-baseline --steps 5 --warmup 2 > $O/acq_$F.log 2>&1
  grep -h "phase" $O/acq_$F.log
  python3 - "$F" "$O" <<'PY'
import json, sys
for l in open(f"{sys.argv[2]}/acq_{sys.argv[1]}.log"):
    if l.startswith("{"):
        d = json.loads(l)
        print(sys.argv[1], d["ms_per_step"], d["roofline"]["kernels_ms_per_step"], d["validated"])
PY
done
