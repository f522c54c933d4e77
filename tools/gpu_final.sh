set -o pipefail
# usage (on the GPU box): TAG=r02o [OUT_DIR=dir] bash tools/gpu_final.sh -> GPU tests + smoke, full metric bench (with CPU
# baseline), per-config full bench lines (1, 2, 3@16spp, 5), light-path variant line, rocprof trace + PMC passes
TAG=${TAG:-r02}
O=${OUT_DIR:-bench_out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 400 --timeout-method thread > $O/gpu_tests_$TAG.log 2>&1 || exit 1
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1 || exit 1
timeout -k 10 300 python -u bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.log || exit 1
for c in 1 2 3 5; do
  timeout -k 10 400 python -u bench.py --full --config $c > $O/bench_cfg${c}_$TAG.json 2> $O/bench_cfg${c}_$TAG.log || exit 1
done
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --bdpt 256,4 --steps 16 --warmup 8 > $O/bench_bdpt_$TAG.json 2> $O/bench_bdpt_$TAG.log || exit 1
OUT_DIR=$O bash tools/profile.sh $TAG trace fetch write sq
