# The shader clock inside the fp16 filter pass, per MFMA shape: builds csrc/topk_scan16.hip with -DTFRS_SCAN16_CLOCKS=1
# into ab/libtfrs_clocks.so (the other objects come from the regular build), then runs the headline batch with it for
# both TFRS_SCAN16_MFMA arms, alternating, and prints per launch (median of the timed launches) the shader cycles, the
# wall time and MHz = cycles / (ticks / 100) of workgroup 0, which lives as long as the launch.
#   tools/exp_scan16_clock.sh build   (no GPU needed)      tools/exp_scan16_clock.sh run
cd "$(dirname "$0")/.."
set -e
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
if [ "${1:-build}" = build ]; then
  python -m recommenders_amd.csrc.build > /dev/null
  mkdir -p ab
  $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-honor-nans -DTFRS_SCAN16_CLOCKS=1 -x hip \
    -c recommenders_amd/csrc/topk_scan16.hip -o ab/topk_scan16_clocks.o
  objs=$(ls recommenders_amd/csrc/_obj/*.o | grep -v '/topk_scan16\.o$')
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o ab/libtfrs_clocks.so $objs ab/topk_scan16_clocks.o
  rm -f ab/topk_scan16_clocks.o
  echo built ab/libtfrs_clocks.so
  exit 0
fi
cp recommenders_amd/libtfrs_hip.so ab/lib_before_clock_run.so
trap 'cp ab/lib_before_clock_run.so recommenders_amd/libtfrs_hip.so' EXIT
cp ab/libtfrs_clocks.so recommenders_amd/libtfrs_hip.so
for rep in 1 2 3; do
  for arm in 32x32 16x16; do
    TFRS_SCAN16_MFMA=$arm timeout -k 10 300 python bench.py --gpus 1 --steps 50 --warmup 10 2>/dev/null | grep '^scan16f_clocks' | tail -50 | \
      python -c "
import sys
rows = [(int(l.split()[6]), int(l.split()[8])) for l in sys.stdin]
med = lambda xs: sorted(xs)[len(xs) // 2]
print('$arm rep $rep: %d launches, median per launch: %d shader cycles, %.1f us, %.0f MHz' % (
    len(rows), med([c for c, t in rows]), med([t for c, t in rows]) / 100.0, med([100.0 * c / t for c, t in rows])))
"
  done
done
