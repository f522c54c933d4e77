set -o pipefail
# usage (on the GPU box): TAG=r03a STEPS="tests smoke bench rays" [OUT_DIR=dir] bash tools/gpu_run.sh
TAG=${TAG:-r03}
O=${OUT_DIR:-bench_out}
mkdir -p $O
for s in ${STEPS:-tests smoke bench}; do
  case $s in
    tests) timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gpu_tests_$TAG.log 2>&1 || exit 1 ;;
    smoke) timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1 || exit 1 ;;
    bench) timeout -k 10 400 python -u bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.log || exit 1 ;;
    drv)   timeout -k 10 400 python -u bench.py --full --steps 20 --warmup 5 > $O/bench_drv_$TAG.json 2> $O/bench_drv_$TAG.log || exit 1 ;;
    rays)  timeout -k 10 300 python -u tools/dump_rays.py $O/rays_$TAG.npz > $O/rays_$TAG.log 2>&1 || exit 1 ;;
    binning) timeout -k 10 120 tools/calib/calib_binning 85000000 40975 5 > $O/binning_85M_$TAG.json && timeout -k 10 120 tools/calib/calib_binning 22500000 40975 5 > $O/binning_22M_$TAG.json || exit 1 ;;
  esac
  echo "step $s done"
done
