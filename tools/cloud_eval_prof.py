"""Wall time of the cloud evaluation's distances: the device path (dpe_cloud_nn_pair in a warm context) against
the host path (dpe_host_cloud_nn in both directions, at most 16 threads), in one run.

The clouds are synthetic.gt_point_cloud of a 4-view scene at two sizes, about 2*10^5 (256 x 192) and 2*10^6
(800 x 600) points per cloud; the second cloud of a pair is the first with every point moved by half a
threshold in a random direction.  tau = 2 pixel footprints (2 * 5 / fx), radius = 2 tau.  A third pair is the
small cloud with 50 000 more points inside ONE cell (a cube of edge 0.4 R): the crowded cell that every one of
its queries walks in full.  Each timing is the best of 5 after one warm-up; the device parts (stage, build,
query, download) are hipEvent milliseconds of the best run (dpe_cloud_last_timings).  Both paths must give the
same bits, which is checked on every size.

Also runs the smallest end-to-end case (64 x 48, 4 views, fusion) and records the F-scores of DPE/DPE.ply
against the scene's ground truth at 1, 2, 4, 8 pixel footprints.

Usage: python tools/cloud_eval_prof.py [--out profiles/cloud_eval.json] [--reps 5]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpe-mvs_amd"))
import numpy as np  # noqa: E402
from DPE_MVS import native, pipeline, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_eval.json"))
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()


def best_of(fn, reps):
    fn()                                   # warm-up
    best, extra = None, None
    for _ in range(reps):
        t = time.perf_counter()
        x = fn()
        dt = time.perf_counter() - t
        if best is None or dt < best:
            best, extra = dt, x
    return best, extra


result = {"host_threads": min(16, os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS") or 16)), "sizes": []}
ctx = native.PatchMatchContext(0)
ctx.set_timing(True)
for W, H, crowd in ((256, 192, 0), (800, 600, 0), (256, 192, 50_000)):
    sc = synthetic.make_scene(W, H, 4)
    A = synthetic.gt_point_cloud(sc)
    del sc
    tau = 2 * 5.0 / (1.2 * W)
    R = 2 * tau
    rng = np.random.default_rng(3)
    if crowd:
        A = np.concatenate([A, (A[0] + rng.random((crowd, 3)) * 0.4 * R).astype(np.float32)])
    u = rng.normal(0, 1, A.shape)
    B = (A + 0.5 * tau * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    host_s, (h_ab, h_ba) = best_of(lambda: (pipeline.cloud_nn(A, B, R), pipeline.cloud_nn(B, A, R)), a.reps)

    def device():
        out = ctx.cloud_nn_pair(A, B, R)
        return out, ctx.cloud_timings()
    dev_s, ((d_ab, d_ba), parts) = best_of(device, a.reps)
    same = bool(np.array_equal(h_ab.view(np.uint32), d_ab.view(np.uint32)) and np.array_equal(h_ba.view(np.uint32), d_ba.view(np.uint32)))
    e = pipeline.evaluate_clouds(A, B, [tau, R])
    row = {"points_per_cloud": int(len(A)), "points_in_one_cell": crowd, "tau": tau, "radius": R, "host_seconds": host_s, "device_seconds": dev_s,
           "device_parts_ms": parts, "identical": same, "fscore": e["fscore"], "precision": e["precision"]}
    result["sizes"].append(row)
    print(json.dumps(row), flush=True)
ctx.close()

folder = tempfile.mkdtemp(prefix="dpe_cloud_eval_prof_")
try:
    sc = synthetic.write_dense_folder(folder, 64, 48, 4)
    pipeline.run_dpe_pipeline(folder, gpu_index=0, verbose=False, fusion=True)
    recon = pipeline.read_point_cloud(os.path.join(folder, pipeline.OUT_NAME, "DPE.ply"))
    foot = 5.0 / (1.2 * 64)
    e = pipeline.evaluate_clouds(recon, synthetic.gt_point_cloud(sc), [foot, 2 * foot, 4 * foot, 8 * foot], gpu_index=0)
    result["end_to_end_64x48x4"] = {k: e[k] for k in ("tau", "precision", "recall", "fscore", "n_recon", "n_gt",
                                                       "mean_accuracy_truncated", "mean_completeness_truncated")}
    print(json.dumps(result["end_to_end_64x48x4"]), flush=True)
finally:
    shutil.rmtree(folder, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written", a.out)
