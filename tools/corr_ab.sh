cd "${GRAFT_REPO_ROOT:-.}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest tests/test_spectral_gpu.py -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT/t5.log 2>&1; tail -2 $OUT/t5.log
for v in ${CORR_VARIANTS:-ab/head.so - ab/head.so - ab/head.so -}; do
  if [ "$v" = "-" ]; then L=algo-dsp_amd/libalgodsp_hip.so; else L=$v; fi
  ALGODSP_LIB=$PWD/$L timeout -k 10 120 python bench.py --workload corr --steps ${CORR_STEPS:-10} --warmup 3 --full > $OUT/corr.json 2>/dev/null || { echo fail $v; exit 1; }
  python -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('$v', d['value'], d['ms_per_step'], d['roofline']['frac'], d.get('parity'))" "$OUT/corr.json"
done
