#!/usr/bin/env python3
"""What the viz medium results cost: the end-to-end dense folder of bench.py's
end_to_end() (10 images of 1600x1200, 9 source views, EdgeSegment computed) run twice with
viz = false and once with viz = true, with dpe_pipeline_last_timings [0] total, [3] passes, [4]
outputs (the viz writer is joined there) and [6] the pass work alone; and the device time of the
viz jobs, measured on an idle stream as enqueue-to-completion of dpe_state_render_jpeg_blocks
(render kernel + JPEG front-half kernel + block copy into a pinned buffer) at the schedule's two
level sizes.  Prints one JSON object; --out also writes it to a file.

    python3 tools/viz_overhead.py --out profiles/viz_overhead.json

--point-cloud all|strong measures the per-image point clouds (point_<it>.ply) the same way instead: the
third run has point_cloud on (viz off), and the job is dpe_state_point_cloud (colour upload, count /
offsets / fill kernels, the count's round trip and the copy of the points into a pinned buffer) plus,
from hipEvents around dpe_point_cloud_arrays' kernels only, nothing else: the kernels' own time is the
job time minus the copies, reported as measured with an empty cloud (depth_max below every depth).

    python3 tools/viz_overhead.py --point-cloud all --out profiles/point_cloud_overhead.json
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpe-mvs_amd"))


def timings(pipeline):
    t = (C.c_double * 8)()
    pipeline.lib().dpe_pipeline_last_timings(t, 8)
    return {"total_s": round(t[0], 4), "passes_s": round(t[3], 4), "outputs_s": round(t[4], 4), "pass_work_s": round(t[6], 4)}


def run_once(pipeline, src, viz, n, W, H, point_cloud=0):
    d = tempfile.mkdtemp(prefix="dpe_viz_")
    try:
        folder = os.path.join(d, "dense")
        shutil.copytree(src, folder)
        t0 = time.perf_counter()
        pipeline.run_dpe_pipeline(folder, verbose=False, viz=viz, point_cloud=point_cloud)
        dt = time.perf_counter() - t0
        made = [os.path.join(b, f) for b, _, fs in os.walk(os.path.join(folder, "DPE")) for f in fs]
        jpgs = sum(f.endswith(".jpg") for f in made)
        plys = [f for f in made if os.path.basename(f).startswith("point_")]
        out = timings(pipeline)
        out.update(viz=viz, point_cloud=point_cloud, wall_s=round(dt, 4), mpix_s=round(n * W * H / dt / 1e6, 4), pictures=jpgs,
                   point_clouds=len(plys), point_cloud_mb=round(sum(os.path.getsize(f) for f in plys) / 1e6, 1))
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def job_device_ms(native, _abi, synthetic, W, H, reps):
    """ms per (image, pass, kind) job at W x H: enqueue to completion on an otherwise idle stream."""
    sc = synthetic.make_scene(W, H, 2)
    p = _abi.default_params()
    p.state = _abi.REFINE_ITER
    p.max_iterations = 1
    inp = synthetic.pass_input(sc, p)
    ctx = native.PatchMatchContext(0)
    lib = native._LIB
    try:
        ctx.stage(inp, synthetic.gt_state(sc))
        ctx.execute()
        ctx.state_save(0)
        buf = np.empty(((W + 15) // 16) * ((H + 15) // 16) * 6 * 64, np.int16)
        pinned = lib.dpe_host_pin(C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes)) == 0
        out = {}
        for kind, name in enumerate(("depth", "normal", "weak")):
            best = None
            for _ in range(reps + 1):                               # the first call allocates
                lib.dpe_sync(ctx._ctx)
                t0 = time.perf_counter()
                rc = lib.dpe_state_render_jpeg_blocks(ctx._ctx, 0, kind, p.depth_min, p.depth_max, 95, buf.ctypes.data, buf.size, None)
                rc = rc or lib.dpe_state_render_wait(ctx._ctx, buf.ctypes.data)
                dt = (time.perf_counter() - t0) * 1e3
                if rc != 0:
                    raise RuntimeError(lib.dpe_last_error().decode())
                best = dt if best is None else min(best, dt)
            out[name] = round(best, 4)
        if pinned:
            lib.dpe_host_unpin(C.c_void_p(buf.ctypes.data))
        out["pinned"] = pinned
        return out
    finally:
        ctx.close()


def point_cloud_job_ms(native, _abi, synthetic, W, H, mode, reps):
    """ms per (image, round) point cloud at W x H on an otherwise idle stream, enqueue to completion: the
    whole job (every pixel of the ground-truth state is a point), and the same call with depth_max below
    every depth (no point, so no copy-out: the colour upload, the three kernels and the count)."""
    sc = synthetic.make_scene(W, H, 2)
    p = _abi.default_params()
    p.state = _abi.REFINE_ITER
    p.max_iterations = 1
    inp = synthetic.pass_input(sc, p)
    ctx = native.PatchMatchContext(0)
    lib = native._LIB
    try:
        ctx.stage(inp, synthetic.gt_state(sc))
        ctx.execute()
        ctx.state_save(0)
        buf = np.empty((W * H, 6), np.float32)
        bgr = np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.uint8)
        pinned = lib.dpe_host_pin(C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes)) == 0
        out = {}
        for name, dmax in (("job", p.depth_max), ("no_points", 0.0)):
            best, n = None, C.c_size_t()
            for _ in range(reps + 1):                               # the first call allocates
                lib.dpe_sync(ctx._ctx)
                t0 = time.perf_counter()
                rc = lib.dpe_state_point_cloud(ctx._ctx, 0, mode, C.byref(sc["cams"][0]), bgr.ctypes.data, p.depth_min, dmax,
                                               buf.ctypes.data, len(buf), C.byref(n), None)
                rc = rc or lib.dpe_state_point_cloud_wait(ctx._ctx, buf.ctypes.data)
                dt = (time.perf_counter() - t0) * 1e3
                if rc != 0:
                    raise RuntimeError(lib.dpe_last_error().decode())
                best = dt if best is None else min(best, dt)
            out[name + "_ms"] = round(best, 4)
            out[name + "_points"] = n.value
        if pinned:
            lib.dpe_host_unpin(C.c_void_p(buf.ctypes.data))
        out["pinned"] = pinned
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=10)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--point-cloud", choices=("all", "strong"), default=None,
                    help="measure the per-image point clouds instead of the viz pictures")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from DPE_MVS import _abi, native, pipeline, synthetic
    n, W, H = a.images, a.width, a.height
    base = tempfile.mkdtemp(prefix="dpe_viz_src_")
    try:
        src = os.path.join(base, "dense")
        synthetic.write_dense_folder(src, W, H, n, max_src=min(9, n - 1), with_edges=False)
        run_once(pipeline, src, False, n, W, H)                    # warm-up: code objects, page cache
        runs = [run_once(pipeline, src, False, n, W, H), run_once(pipeline, src, False, n, W, H),
                run_once(pipeline, src, True, n, W, H) if a.point_cloud is None else
                run_once(pipeline, src, False, n, W, H, pipeline.POINT_CLOUD_MODES[a.point_cloud])]
    finally:
        shutil.rmtree(base, ignore_errors=True)
    rounds, m = 1, max(W, H)
    while m > 800:
        m //= 2
        rounds += 1
    rounds = max(rounds, 2)
    levels, device_s = {}, 0.0
    for i in range(rounds):
        s = 1 << (rounds - 1 - i)
        w, h = pipeline.std_round(W / s), pipeline.std_round(H / s)
        if a.point_cloud is not None:                               # one job per image and round
            ms = point_cloud_job_ms(native, _abi, synthetic, w, h, pipeline.POINT_CLOUD_MODES[a.point_cloud], a.reps)
            levels[f"{w}x{h}"] = ms
            device_s += n * ms["job_ms"] / 1e3
            continue
        ms = job_device_ms(native, _abi, synthetic, w, h, a.reps)
        levels[f"{w}x{h}"] = ms
        device_s += n * 4 * (ms["depth"] + ms["normal"] + ms["weak"]) / 1e3
    off = [r["pass_work_s"] for r in runs[:2]]
    what = "viz" if a.point_cloud is None else "point_cloud"
    res = {"images": n, "width": W, "height": H, "runs": runs, what + "_job_ms": levels,
           what + "_device_s_per_run": round(device_s, 4),
           "pass_work_%s_off_s" % what: off, "pass_work_%s_on_s" % what: runs[2]["pass_work_s"],
           "pass_work_bound_s": round(max(off) + abs(off[0] - off[1]) + device_s, 4),
           "pass_work_within_bound": runs[2]["pass_work_s"] <= max(off) + abs(off[0] - off[1]) + device_s}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
