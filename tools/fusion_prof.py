"""Where fusion's time goes at BASELINE configs[4] (bench.py pipeline_config5).

Default: runs the config-5 pipeline once on GPU 0 with DPE_FUSION_PROFILE=1, which prints the seconds
RunFusion spends waiting for the candidate copies, in the parallel angle / weight terms and in the
serial walk (host/fusion.cpp).

--mode tat_intermediate | tat_advanced | both: the Tanks-and-Temples fusions.  Runs the same pipeline
once keeping the final maps, then times, over those maps, the reference's serial loops (the yardstick,
host/fusion_tat.cpp) against the device path the pipeline takes (dpe_fusion_tat_image), alternating the
two `--reps` times after one untimed device run, and checks that both give the same points.  Each time
is a host clock around one whole fusion (the device one includes its context, the uploads of depths,
normals, colours and the copy-out of the points).

--consistency N: the pipeline run also writes the consistency maps with min_views = N, and the line it
prints carries dpe_pipeline_last_timings [8] (views, staging, one kernel and 5 B/px back per image, the
two .npy files) beside [7] (RunFusion, whose candidates path brings 16 * ns B/px back): the filter's cost
against the candidates path on the same folder, in the same run.
Usage: python tools/fusion_prof.py [n_images] [width] [height] [--mode M] [--reps R] [--consistency N]"""
import argparse
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpe-mvs_amd"))
os.environ["DPE_FUSION_PROFILE"] = "1"
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
from DPE_MVS import pipeline, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=32)
ap.add_argument("W", nargs="?", type=int, default=1920)
ap.add_argument("H", nargs="?", type=int, default=1080)
ap.add_argument("--mode", choices=["eth3d", "tat_intermediate", "tat_advanced", "both"], default="eth3d")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--consistency", type=int, default=0, metavar="N")
a = ap.parse_args()
n, W, H = a.n, a.W, a.H


def final_views(folder):
    """The views fusion reads: pair.txt order, final maps of a keep_intermediate run."""
    tok = open(os.path.join(folder, "pair.txt")).read().split()
    pos, views = 1, []
    for _ in range(int(tok[0])):
        ref, k = int(tok[pos]), int(tok[pos + 1])
        src = [int(tok[pos + 2 + 2 * q]) for q in range(k) if float(tok[pos + 3 + 2 * q]) > 0]
        pos += 2 + 2 * k
        rf = os.path.join(folder, pipeline.OUT_NAME, f"{ref:08d}")
        dep = pipeline.read_bin_mat(os.path.join(rf, "depths.dmb"))
        cam = pipeline.read_camera(os.path.join(folder, "cams", f"{ref:08d}_cam.txt"))
        cam.width, cam.height = dep.shape[1], dep.shape[0]
        views.append(dict(image_id=ref, src_ids=src, cam=cam, depth=dep,
                          normal=pipeline.read_bin_mat(os.path.join(rf, "normals.dmb")),
                          bgr=pipeline.read_bgr(os.path.join(folder, "images", f"{ref:08d}.jpg")), block=None))
    return views


folder = f"/tmp/dpe_fusion_prof_{os.getpid()}"
try:
    sc = synthetic.make_scene(W, H, n)
    synthetic.write_dense_folder(folder, W, H, n, max_src=min(31, n - 1), with_edges=False, scene=sc)
    del sc
    print("scene written", flush=True)
    t0 = time.perf_counter()
    pipeline.run_dpe_pipeline(folder, gpu_index=0, verbose=False, fusion=True, keep_intermediate=a.mode != "eth3d",
                              consistency=a.consistency)
    import ctypes
    ph = (ctypes.c_double * 9)()
    pipeline.lib().dpe_pipeline_last_timings(ph, 9)
    print(f"{n} x {W}x{H}: wall {time.perf_counter() - t0:.2f} s, passes {ph[6]:.2f} s, fusion {ph[7]:.2f} s" +
          (f", consistency maps (min_views {a.consistency}) {ph[8]:.3f} s" if a.consistency else ""), flush=True)
    if a.consistency:   # what the maps say, so that the time above is the time of a real answer
        hist, kept = np.zeros(256, np.int64), 0
        for i in range(n):
            rf = os.path.join(folder, pipeline.OUT_NAME, f"{i:08d}")
            hist += np.bincount(np.load(os.path.join(rf, "consistency.npy")).ravel(), minlength=256)
            kept += np.count_nonzero(np.load(os.path.join(rf, "depth_filtered.npy")))
        top = int(np.nonzero(hist)[0].max())
        print(f"consistency: {kept} of {n * W * H} pixels kept ({100.0 * kept / (n * W * H):.1f} %), "
              f"count histogram 0..{top}: {hist[:top + 1].tolist()}", flush=True)
    if a.mode != "eth3d":
        views = final_views(folder)
        for mode in (["tat_intermediate", "tat_advanced"] if a.mode == "both" else [a.mode]):
            _, _, cnt = pipeline.fusion_tat_run(views, mode, gpu_index=0, cap=0)     # untimed: code objects, count
            print(f"{mode}: {cnt} points", flush=True)
            ts, td, same = [], [], True
            for r in range(a.reps):
                t = time.perf_counter()
                ps, _, cs = pipeline.fusion_tat_run(views, mode, gpu_index=-1, cap=cnt)
                ts.append(time.perf_counter() - t)
                t = time.perf_counter()
                pd, _, cd = pipeline.fusion_tat_run(views, mode, gpu_index=0, cap=cnt)
                td.append(time.perf_counter() - t)
                same = same and cs == cd == cnt and np.array_equal(ps.view(np.uint32), pd.view(np.uint32))
                print(f"  rep {r}: serial {ts[-1]:.3f} s, device {td[-1]:.3f} s, identical {same}", flush=True)
            print(f"{mode} at {n} x {W}x{H}: serial median {np.median(ts):.3f} s (min {min(ts):.3f}, max {max(ts):.3f}), "
                  f"device median {np.median(td):.3f} s (min {min(td):.3f}, max {max(td):.3f}), "
                  f"{np.median(ts) / np.median(td):.1f}x, points identical: {same}", flush=True)
finally:
    shutil.rmtree(folder, ignore_errors=True)
