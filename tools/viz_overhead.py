#!/usr/bin/env python3
"""What the viz medium results cost: the end-to-end dense folder of bench.py's
end_to_end() (10 images of 1600x1200, 9 source views, EdgeSegment computed) run twice with
viz = false and once with viz = true, with dpe_pipeline_last_timings [0] total, [3] passes, [4]
outputs (the viz writer is joined there) and [6] the pass work alone; and the device time of the
viz jobs, measured on an idle stream as enqueue-to-completion of dpe_state_render_jpeg_blocks
(render kernel + JPEG front-half kernel + block copy into a pinned buffer) at the schedule's two
level sizes.  Prints one JSON object; --out also writes it to a file.

    python3 tools/viz_overhead.py --out profiles/viz_overhead.json
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


def run_once(pipeline, src, viz, n, W, H):
    d = tempfile.mkdtemp(prefix="dpe_viz_")
    try:
        folder = os.path.join(d, "dense")
        shutil.copytree(src, folder)
        t0 = time.perf_counter()
        pipeline.run_dpe_pipeline(folder, verbose=False, viz=viz)
        dt = time.perf_counter() - t0
        jpgs = sum(f.endswith(".jpg") for _, _, fs in os.walk(os.path.join(folder, "DPE")) for f in fs)
        out = timings(pipeline)
        out.update(viz=viz, wall_s=round(dt, 4), mpix_s=round(n * W * H / dt / 1e6, 4), pictures=jpgs)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=10)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
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
                run_once(pipeline, src, True, n, W, H)]
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
        ms = job_device_ms(native, _abi, synthetic, w, h, a.reps)
        levels[f"{w}x{h}"] = ms
        device_s += n * 4 * (ms["depth"] + ms["normal"] + ms["weak"]) / 1e3
    off = [r["pass_work_s"] for r in runs[:2]]
    res = {"images": n, "width": W, "height": H, "runs": runs, "viz_job_ms": levels,
           "viz_device_s_per_run": round(device_s, 4),
           "pass_work_viz_off_s": off, "pass_work_viz_on_s": runs[2]["pass_work_s"],
           "pass_work_bound_s": round(max(off) + abs(off[0] - off[1]) + device_s, 4),
           "pass_work_within_bound": runs[2]["pass_work_s"] <= max(off) + abs(off[0] - off[1]) + device_s}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
