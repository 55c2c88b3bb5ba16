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

With --voxel V the tool measures the voxel down-sampling instead (dpe_cloud_voxel in a warm context against the
serial host loop dpe_host_cloud_voxel) on the 800 x 600 pair, 1.92 million points each, at voxel edge V, and writes
profiles/cloud_voxel.json: the device time by part (stage, cells + insert, emit, download: dpe_cloud_last_timings),
the host loop's time, the bytes of device scratch per point, the cells + insert part on the 24 096 points of the
tests' line cloud, whose crowd of 20 000 shares ONE voxel at edge 0.01, and on the same cloud without the crowd (what
contention on one slot costs), and the 64 x 48 end-to-end F-scores with both clouds down-sampled at tau_max / 2.

With --voxel V --ab LIB LIB... it instead compares builds of libdpe_mvs.so (tools/build_variants.sh) on the
down-sampling, interleaved in one process: the cells + insert part and the whole call's wall time per build on the
800 x 600 cloud and on the two line clouds, every build held to the first one's records.

With --register R the tool measures the ICP step instead (dpe_cloud_icp_stage / dpe_cloud_icp_step in a warm context
against dpe_host_cloud_icp_step) on the 800 x 600 pair, target A and source B moved by the inverse of the tests'
(R0, t0) (4 degrees about (1, 2, 3), shift (0.03, -0.02, 0.01)), at match radius R, and writes
profiles/cloud_register.json: the wall time of one device step and of one host step under the true transform (median
and spread of --reps runs after a warm-up; the host step includes the build of the target's grid, which the device
stages once), the step's device parts (apply + build, match, sums, download: dpe_cloud_last_timings), the kernels
launched per step, and a loop driven from here, step by step with the host's solve, from a start within reach of R
(the true transform turned by 0.02 degrees and shifted by R / 4) to the fixed point: the number of steps and every
step's parts.  The radius of a whole-scene 4 degree error (0.35 here) is out of the grid's reach at this density, so
the loop from the identity is not what is timed.

With --render the tool measures the depth-map evaluation instead (dpe_cloud_render_stage once, then
dpe_cloud_render_view and dpe_depth_score per view in a warm context, against dpe_host_cloud_render on at most 16
host threads and the serial dpe_host_depth_score): the 800 x 600 scene's cloud, 1.92 million points, into 10 views
at 1600 x 1200 on an arc around the scene, with splat half-widths 0 and 2, the estimate being the rendered map with
1 % noise, and writes profiles/depth_render.json: the staging's wall time and upload part, and per half-width the
device parts of a view (render, score with its upload, download: dpe_cloud_last_timings) and the wall time of a view
on either path, each as median, min and max over views and --reps runs after a warm-up.  Both paths must give the same
bits, which is checked on every view.  The contention case is 10^6 points on ONE pixel of a 1600 x 1200 view (their
depths a permutation, so the minimum keeps falling) against 10^6 points of the scene's cloud in the same view.

With --normals R the tool measures the normal-map evaluation instead and writes profiles/cloud_normals.json.  Point
normals: dpe_cloud_normals in a warm context against dpe_host_cloud_normals (at most 16 host threads) on the two cloud
sizes above, at radius R (R = 0: the radius of the distances above, 2 tau = 4 pixel footprints), with the device parts
(stage, build, normals, download: dpe_cloud_last_timings), and beside the normals part the match part of
dpe_cloud_nn_index of the cloud against itself at the same radius: k_cloud_match makes the same walk, so the ratio
prices the ten sums and the solve.  Render: the 800 x 600 cloud staged with its normals, then dpe_cloud_render_view_normals
and dpe_cloud_render_view into the --render views' middle camera at 1600 x 1200 with half-widths 0 and 2 (the render part
of each), and the host render with normals.  Score: dpe_normal_score of a 1600 x 1200 map against the rendered one with
noise, and of a map of ONE plane (every pixel of a wave in one bin of the block's LDS histogram), against the serial host
score.  Both paths must give the same bits, which is checked on every case.

Usage: python tools/cloud_eval_prof.py [--out profiles/cloud_eval.json] [--reps 5] [--voxel V [--ab LIB LIB...]] [--register R] [--render]
       [--normals R]"""
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
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--voxel", type=float, default=None, help="measure the voxel down-sampling at this edge instead")
ap.add_argument("--ab", nargs="+", default=None, help="with --voxel: builds of libdpe_mvs.so to compare, interleaved")
ap.add_argument("--register", type=float, default=None, help="measure the ICP step at this match radius instead")
ap.add_argument("--render", action="store_true", help="measure the depth-map evaluation (render and score) instead")
ap.add_argument("--normals", type=float, default=None, help="measure the normal-map evaluation at this PCA radius instead (0: 2 tau)")
a = ap.parse_args()
a.out = a.out or os.path.join(ROOT, "profiles", "cloud_normals.json" if a.normals is not None else "depth_render.json" if a.render else "cloud_register.json" if a.register is not None else
                              "cloud_eval.json" if a.voxel is None else "cloud_voxel.json")


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


def same_records(x, y):
    return all((p is None and q is None) or (p.dtype == q.dtype and p.tobytes() == q.tobytes()) for p, q in zip(x, y))


def line_cloud():
    """The target of the tests' line cloud (tests/test_cloud_eval.py): 4 096 points along one axis and a crowd of
    20 000 inside one cell of edge 0.01; returns (all of it, the line alone)."""
    R = 0.01
    rng = np.random.default_rng(9)
    line = np.zeros((4096, 3))
    line[:, 0] = np.sort(rng.random(4096)) * 1e4 * R
    line[:, 1:] = rng.random((4096, 2)) * 0.5 * R
    crowd = np.array([50.25 * R, 0.1 * R, 0.1 * R]) + rng.random((20000, 3)) * 0.4 * R
    return np.concatenate([line, crowd]).astype(np.float32), line.astype(np.float32)


def voxel_profile():
    out = {"voxel": a.voxel, "clouds": []}
    live0 = native.live_device_bytes()
    ctx = native.PatchMatchContext(0)
    ctx.set_timing(True)
    sc = synthetic.make_scene(800, 600, 4)
    A = synthetic.gt_point_cloud(sc)
    del sc
    rng = np.random.default_rng(3)
    tau = 2 * 5.0 / (1.2 * 800)
    u = rng.normal(0, 1, A.shape)
    B = (A + 0.5 * tau * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    col = rng.integers(0, 256, A.shape).astype(np.uint8)
    for name, P, C in (("A", A, None), ("B", B, None), ("A with colours", A, col)):
        host_s, h = best_of(lambda: pipeline.voxel_down_sample(P, a.voxel, C), max(1, a.reps // 2))

        def device():
            r = ctx.cloud_voxel(P, a.voxel, C)
            return r, ctx.cloud_timings()
        dev_s, (d, parts) = best_of(device, a.reps)
        parts = dict(zip(("stage", "cells_insert", "emit", "download"), parts.values()))
        row = {"cloud": name, "points": int(len(P)), "voxels": int(len(d[0])), "largest_voxel": int(d[3].max()),
               "host_seconds": host_s, "device_seconds": dev_s, "device_parts_ms": parts, "identical": same_records(h, d)}
        out["clouds"].append(row)
        print(json.dumps(row), flush=True)
    out["scratch_bytes_per_point_with_colours"] = (native.live_device_bytes() - live0) / len(A)
    full, line = line_cloud()
    for name, P in (("line cloud, 20 000 points in one voxel", full), ("line cloud without that voxel", line)):

        def device():
            r = ctx.cloud_voxel(P, 0.01)
            return r, ctx.cloud_timings()
        dev_s, (d, parts) = best_of(device, a.reps)
        parts = dict(zip(("stage", "cells_insert", "emit", "download"), parts.values()))
        row = {"cloud": name, "points": int(len(P)), "voxels": int(len(d[0])), "largest_voxel": int(d[3].max()),
               "device_seconds": dev_s, "device_parts_ms": parts, "identical": same_records(pipeline.voxel_down_sample(P, 0.01), d)}
        out["clouds"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    folder = tempfile.mkdtemp(prefix="dpe_cloud_voxel_prof_")
    try:
        sc = synthetic.write_dense_folder(folder, 64, 48, 4)
        pipeline.run_dpe_pipeline(folder, gpu_index=0, verbose=False, fusion=True)
        recon = pipeline.read_point_cloud(os.path.join(folder, pipeline.OUT_NAME, "DPE.ply"))
        foot = 5.0 / (1.2 * 64)
        e = pipeline.evaluate_clouds(recon, synthetic.gt_point_cloud(sc), [foot, 2 * foot, 4 * foot, 8 * foot], gpu_index=0, voxel=4 * foot)
        out["end_to_end_64x48x4_voxel_half_tau_max"] = {k: e[k] for k in ("tau", "voxel", "precision", "recall", "fscore", "n_recon_in", "n_gt_in",
                                                                          "n_recon", "n_gt")}
        print(json.dumps(out["end_to_end_64x48x4_voxel_half_tau_max"]), flush=True)
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    return out


def voxel_ab(paths):
    import ctypes as C
    sc = synthetic.make_scene(800, 600, 4)
    A = synthetic.gt_point_cloud(sc)
    del sc
    col = np.random.default_rng(3).integers(0, 256, A.shape).astype(np.uint8)
    full, line = line_cloud()
    clouds = (("A", A, None, a.voxel), ("A with colours", A, col, a.voxel), ("line cloud, 20 000 points in one voxel", full, None, 0.01),
              ("line cloud without that voxel", line, None, 0.01))
    libs = [(p, native.load_library(p)) for p in paths]
    ctxs = [(p, L, L.dpe_create(0)) for p, L in libs]
    for _, L, c in ctxs:
        L.dpe_set_timing(c, 1)
    out = {"voxel": a.voxel, "rounds": a.reps, "builds": paths, "clouds": []}
    for name, P, Cc, v in clouds:
        n = len(P)
        xyz, rgb, first, count = np.empty((n, 3), np.float32), np.empty((n, 3), np.uint8), np.empty(n, np.int32), np.empty(n, np.int32)
        k, ms = C.c_size_t(), (C.c_float * 4)()
        ref, rows = None, {p: {"cells_insert_ms": [], "wall_ms": []} for p in paths}
        for rnd in range(a.reps + 1):                      # round 0 warms up
            for p, L, c in ctxs:
                t = time.perf_counter()
                rc = L.dpe_cloud_voxel(c, P.ctypes.data, n, None if Cc is None else Cc.ctypes.data, v, xyz.ctypes.data,
                                       None if Cc is None else rgb.ctypes.data, first.ctypes.data, count.ctypes.data, n, C.byref(k))
                dt = time.perf_counter() - t
                assert rc == 0, (p, L.dpe_last_error())
                got = b"".join(x[:k.value].tobytes() for x in ((xyz, first, count) if Cc is None else (xyz, rgb, first, count)))
                ref = ref or got
                assert got == ref, f"{p}: records differ from {paths[0]}"
                L.dpe_cloud_last_timings(c, ms, 4)
                if rnd:
                    rows[p]["cells_insert_ms"].append(float(ms[1]))
                    rows[p]["wall_ms"].append(dt * 1e3)
        row = {"cloud": name, "points": n, "voxels": int(k.value)}
        for p in paths:
            row[os.path.basename(p)] = {key: {"min": min(vals), "median": float(np.median(vals))} for key, vals in rows[p].items()}
        out["clouds"].append(row)
        print(json.dumps(row), flush=True)
    for _, L, c in ctxs:
        L.dpe_destroy(c)
    return out


def rotation(axis, degrees):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def register_profile():
    R = a.register
    PARTS = ("apply_build", "match", "sums", "download")
    sc = synthetic.make_scene(800, 600, 4)
    A = synthetic.gt_point_cloud(sc)
    del sc
    rng = np.random.default_rng(3)
    tau = 2 * 5.0 / (1.2 * 800)
    u = rng.normal(0, 1, A.shape)
    B = (A + 0.5 * tau * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    R0, t0 = rotation([1, 2, 3], 4.0), np.array([0.03, -0.02, 0.01])
    src = ((B.astype(np.float64) - t0) @ R0).astype(np.float32)             # B under (R0, t0)^-1
    true = np.concatenate([R0, t0[:, None]], axis=1)
    out = {"radius": R, "points_per_cloud": int(len(A)), "host_threads": min(16, os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS") or 16)),
           "reps": a.reps}
    ctx = native.PatchMatchContext(0)
    ctx.set_timing(True)
    t = time.perf_counter()
    ctx.cloud_icp_stage(src, A, R)
    out["device_stage_seconds_cold"] = time.perf_counter() - t
    ctx.cloud_icp_step(true)                                                # warm-up
    dev, parts, launches = [], [], []
    for _ in range(a.reps):
        l0 = native.cloud_launches()
        t = time.perf_counter()
        d = ctx.cloud_icp_step(true)
        dev.append(time.perf_counter() - t)
        launches.append(native.cloud_launches() - l0)
        parts.append(dict(zip(PARTS, ctx.cloud_timings().values())))
    pipeline.cloud_icp_step(src, A, R, true)                                # warm-up
    host = []
    for _ in range(max(1, a.reps)):
        t = time.perf_counter()
        h = pipeline.cloud_icp_step(src, A, R, true)
        host.append(time.perf_counter() - t)
    out["identical"] = bool(d == h)
    out["matched"] = d["matched"]
    out["device_step_seconds"] = {"median": float(np.median(dev)), "min": min(dev), "max": max(dev)}
    out["host_step_seconds"] = {"median": float(np.median(host)), "min": min(host), "max": max(host)}
    out["device_parts_ms"] = {k: {"median": float(np.median([p[k] for p in parts])), "min": min(p[k] for p in parts),
                                  "max": max(p[k] for p in parts)} for k in PARTS}
    out["launches_per_step"] = sorted(set(launches))
    print(json.dumps(out), flush=True)
    # the loop from a start within reach of R, driven step by step so that every step's parts are seen
    fin_s, fin_t = np.isfinite(src).all(axis=1), np.isfinite(A).all(axis=1)
    o_s, o_t = src[fin_s].astype(np.float64).min(axis=0), A[fin_t].astype(np.float64).min(axis=0)
    near = rotation([0, 1, 0], 0.02)
    T = np.concatenate([near @ R0, (near @ t0 + R / 4)[:, None]], axis=1)
    prev, steps, fixed = None, [], False
    t = time.perf_counter()
    for it in range(1, 201):
        s = ctx.cloud_icp_step(T)
        steps.append(dict(zip(PARTS, ctx.cloud_timings().values()), matched=s["matched"], rms=float(np.sqrt(s["d2"] / max(1, s["matched"])))))
        T = pipeline.cloud_solve(s, o_s, o_t)
        fixed = s == prev
        if fixed:
            break
        prev = s
    out["loop"] = {"start": "true transform turned by 0.02 degrees about y and shifted by R / 4", "steps_to_fixed_point": it,
                   "reached_fixed_point": fixed, "wall_seconds": time.perf_counter() - t,
                   "final_T_minus_true_max": float(np.abs(T - true).max()), "steps": steps}
    print(json.dumps({k: v for k, v in out["loop"].items() if k != "steps"}), flush=True)
    ctx.close()
    return out


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def arc_cameras(n, W, H):
    """n cameras at W x H on the synthetic scene's arc (synthetic.make_scene), -15 to 15 degrees"""
    import math
    fx = 1.2 * W
    K = np.array([[fx, 0, W / 2.0], [0, fx, H / 2.0], [0, 0, 1.0]])
    O = np.array([0.0, 0.0, 5.0])
    cams = []
    for i in range(n):
        th = math.radians(-15.0 + 30.0 * i / max(1, n - 1))
        Cc = O + 5.0 * np.array([math.sin(th), 0.25 * math.sin(1.7 * i) / 5.0, -math.cos(th)])
        R = synthetic._look_at(Cc, O)
        cams.append(synthetic.make_camera(K, R, -R @ Cc, W, H, 1.0, 20.0))
    return cams


def render_profile():
    W, H, V, TAUS = 1600, 1200, 10, [1e-3, 1e-2]
    sc = synthetic.make_scene(800, 600, 4)
    P = synthetic.gt_point_cloud(sc)
    del sc
    cams = arc_cameras(V, W, H)
    out = {"points": int(len(P)), "views": V, "size": [W, H], "reps": a.reps,
           "host_threads": min(16, os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS") or 16)), "splats": []}
    ctx = native.PatchMatchContext(0)
    ctx.set_timing(True)
    ctx.cloud_render_stage(P)                                              # warm-up: the allocation
    stage_wall, stage_ms = [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        ctx.cloud_render_stage(P)
        stage_wall.append(time.perf_counter() - t)
        stage_ms.append(ctx.cloud_timings()["stage"])
    out["stage_seconds"], out["stage_upload_ms"] = spread(stage_wall), spread(stage_ms)
    rng = np.random.default_rng(4)
    for s in (0, 2):
        row = {"splat": s, "identical": True}
        host_maps, ests, host_render, host_score, host_scores = [], [], [], [], []
        for cam in cams:
            t = time.perf_counter()
            g = pipeline.render_cloud(P, cam, s)
            host_render.append(time.perf_counter() - t)
            e = (g * (1 + 0.01 * rng.standard_normal(g.shape))).astype(np.float32)
            t = time.perf_counter()
            host_scores.append(pipeline.score_depth(e, g, TAUS, relative=True))
            host_score.append(time.perf_counter() - t)
            host_maps.append(g)
            ests.append(e)
        row["coverage"] = float(np.mean([(g > 0).mean() for g in host_maps]))
        render_ms, score_ms, upload_ms, download_ms, view_wall = [], [], [], [], []
        for r in range(a.reps + 1):                                        # the first round is the warm-up
            for cam, g, e, hs in zip(cams, host_maps, ests, host_scores):
                t = time.perf_counter()
                ctx.cloud_render_view(cam, s, download=False)
                tr = ctx.cloud_timings()
                d = ctx.depth_score(e, None, TAUS, relative=True)
                wall = time.perf_counter() - t
                ts = ctx.cloud_timings()
                if r == 0:
                    got = ctx.cloud_render_view(cam, s)
                    d.update(pipeline.depth_stats(d))
                    row["identical"] = bool(row["identical"] and got.tobytes() == g.tobytes() and d == hs)
                    continue
                render_ms.append(tr["build"])
                upload_ms.append(ts["stage"])
                score_ms.append(ts["query"])
                download_ms.append(ts["download"])
                view_wall.append(wall)
        row["device_parts_ms"] = {"render": spread(render_ms), "score_upload": spread(upload_ms), "score": spread(score_ms),
                                  "score_download": spread(download_ms)}
        row["device_view_seconds"] = spread(view_wall)
        row["host_render_seconds"], row["host_score_seconds"] = spread(host_render), spread(host_score)
        out["splats"].append(row)
        print(json.dumps(row), flush=True)
    # contention: every point on one pixel against as many points of the scene
    n = 1_000_000
    d = np.random.default_rng(2).permutation(n).astype(np.float32) * np.float32(2 ** -16) + np.float32(1)
    pixel = synthetic.make_camera(np.eye(3), np.eye(3), np.zeros(3), W, H, 0.1, 100.0)
    crowd = np.stack([np.float32(800) * d, np.float32(600) * d, d], -1).astype(np.float32)
    out["contention"] = []
    for name, pts, cam in (("one_pixel", crowd, pixel), ("scene", P[:n], cams[V // 2])):
        ctx.cloud_render_stage(pts)
        for s in (0, 2):
            ms = []
            for r in range(a.reps + 1):
                got = ctx.cloud_render_view(cam, s, download=(r == 0))
                if r:
                    ms.append(ctx.cloud_timings()["build"])
                else:
                    same = bool(got.tobytes() == pipeline.render_cloud(pts, cam, s).tobytes())
            row = {"cloud": name, "points": int(len(pts)), "splat": s, "render_ms": spread(ms), "identical": same}
            out["contention"].append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    return out


def normals_profile():
    out = {"reps": a.reps, "host_threads": min(16, os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS") or 16)), "sizes": []}
    ctx = native.PatchMatchContext(0)
    ctx.set_timing(True)
    A = nrm = None
    for W, H in ((256, 192), (800, 600)):
        sc = synthetic.make_scene(W, H, 4)
        A = synthetic.gt_point_cloud(sc)
        del sc
        R = a.normals if a.normals > 0 else 4 * 5.0 / (1.2 * W)
        t = time.perf_counter()
        h_nrm, h_cnt = pipeline.estimate_normals(A, R)
        host_s = time.perf_counter() - t

        def device():
            r = ctx.cloud_normals(A, R)
            return r, ctx.cloud_timings()
        dev_s, ((nrm, cnt), parts) = best_of(device, a.reps)
        parts = dict(zip(("stage", "build", "normals", "download"), parts.values()))

        def match():
            ctx.cloud_nn_index(A, A, R)
            return ctx.cloud_timings()["query"]
        match_ms = best_of(match, a.reps)[1]
        row = {"points": int(len(A)), "radius": R, "mean_neighbours": float(cnt.mean()), "max_neighbours": int(cnt.max()),
               "with_normal": float(nrm.any(axis=1).mean()), "host_seconds": host_s, "device_seconds": dev_s, "device_parts_ms": parts,
               "match_ms_same_cloud_and_radius": match_ms, "normals_over_match": parts["normals"] / match_ms,
               "identical": bool(nrm.tobytes() == h_nrm.tobytes() and np.array_equal(cnt, h_cnt))}
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
    # the render: the 800 x 600 cloud and its normals into one 1600 x 1200 view
    Wv, Hv = 1600, 1200
    cam = arc_cameras(10, Wv, Hv)[5]
    ctx.cloud_render_stage(A, nrm)
    out["render"] = []
    gt = None
    for s in (0, 2):
        t = time.perf_counter()
        h_depth, h_normal = pipeline.render_cloud_normals(A, nrm, cam, s)
        host_s = time.perf_counter() - t
        with_ms, plain_ms = [], []
        for r in range(a.reps + 1):                                        # the first round is the warm-up
            depth, normal = ctx.cloud_render_view_normals(cam, s, download=(r == 0))
            if r == 0:
                same = bool(depth.tobytes() == h_depth.tobytes() and normal.tobytes() == h_normal.tobytes())
            else:
                with_ms.append(ctx.cloud_timings()["build"])
            ctx.cloud_render_view(cam, s, download=False)
            if r:
                plain_ms.append(ctx.cloud_timings()["build"])
        row = {"splat": s, "size": [Wv, Hv], "points": int(len(A)), "coverage": float((h_depth > 0).mean()),
               "with_normal": float(h_normal.any(axis=2).mean()), "render_with_normals_ms": spread(with_ms), "render_plain_ms": spread(plain_ms),
               "host_render_with_normals_seconds": host_s, "identical": same}
        out["render"].append(row)
        print(json.dumps(row), flush=True)
        gt = h_normal
    # the score: a noisy copy of the rendered map, and one plane
    rng = np.random.default_rng(4)
    cos_taus = [pipeline.normal_cos(v) for v in (11.25, 22.5, 30.0)]
    noisy = (gt + 0.1 * rng.standard_normal(gt.shape)).astype(np.float32)
    plane_gt = np.tile(np.array([(0, 0, -1)], np.float32), (Hv, Wv, 1))
    plane_est = np.tile(np.array([(0.6, 0, -0.8)], np.float32), (Hv, Wv, 1))
    out["score"] = []
    for name, e, g in (("rendered map with noise", noisy, gt), ("one plane: every pixel in one bin", plane_est, plane_gt)):
        t = time.perf_counter()
        hs = pipeline.score_normals(e, g, cos_taus=cos_taus)
        host_s = time.perf_counter() - t
        score_ms, upload_ms, wall = [], [], []
        for r in range(a.reps + 1):
            t = time.perf_counter()
            d = ctx.normal_score(e, g, cos_taus)
            dt = time.perf_counter() - t
            if r == 0:
                d.update(pipeline.normal_stats(d))
                same = bool(d == hs)
                continue
            ts = ctx.cloud_timings()
            score_ms.append(ts["query"])
            upload_ms.append(ts["stage"])
            wall.append(dt)
        row = {"case": name, "pixels": Wv * Hv, "n_both": hs["n_both"], "largest_bin": max(hs["hist"]), "score_ms": spread(score_ms),
               "upload_ms": spread(upload_ms), "device_seconds": spread(wall), "host_seconds": host_s, "identical": same}
        out["score"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    return out


if a.normals is not None:
    result = normals_profile()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("written", a.out)
    sys.exit(0)

if a.render:
    result = render_profile()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("written", a.out)
    sys.exit(0)

if a.register is not None:
    result = register_profile()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("written", a.out)
    sys.exit(0)

if a.voxel is not None:
    result = voxel_ab(a.ab) if a.ab else voxel_profile()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("written", a.out)
    sys.exit(0)

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
