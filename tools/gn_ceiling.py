"""Timing experiment: the pass without GenNeighbours on its critical path (a -DDPE_DIAG=64 build of
libdpe_mvs.so).

In that build the first execute after a stage runs GenNeighbours and keeps its outputs; later
executes of the same staged state skip it.  This script checks that a later execute gives the same
bits as the first one (GenNeighbours depends only on the staged state), then prints the mean wall
time of the later executes.  Run it once on the diagnostic build and once on a plain one
(tools/build_variants.sh "gnonce:-DDPE_DIAG=64" "base:"); the difference is the ceiling.
Usage: python tools/gn_ceiling.py lib/variants/gnonce.so [reps]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dpe-mvs_amd"))
import torch  # noqa: E402
torch.cuda.set_device(0)
import bench  # noqa: E402
from DPE_MVS import _abi, native, synthetic  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
sc = synthetic.make_scene(1600, 1200, 10)
p = bench.workload_params(_abi, 10)
inp = synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc))
st = synthetic.gt_state(sc)
lib = native.load_library(sys.argv[1])
ctx = lib.dpe_create(0)
bufs = _abi.PassBuffers(inp, st)
assert lib.dpe_pm_stage(ctx, C.byref(bufs.inp), C.byref(bufs.st)) == 0, lib.dpe_last_error()


def run():
    assert lib.dpe_pm_execute(ctx, None) == 0, lib.dpe_last_error()
    assert lib.dpe_pm_fetch(ctx, C.byref(bufs.st)) == 0, lib.dpe_last_error()
    return b''.join(a.tobytes() for a in (bufs.planes, bufs.weak, bufs.sel, bufs.costs))


first = run()
second = run()
assert first == second, "an execute after the first gives different bits"
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(reps):
    assert lib.dpe_pm_execute(ctx, None) == 0, lib.dpe_last_error()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / reps * 1e3
print(f"{os.path.basename(sys.argv[1])}: {dt:.3f} ms per execute ({reps} reps), "
      "bits of execute 2 == execute 1", flush=True)
lib.dpe_destroy(ctx)
