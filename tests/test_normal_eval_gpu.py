"""Normal-map evaluation on the device (csrc/pass_normals.h; dpe_cloud_normals, dpe_cloud_render_stage_normals,
dpe_cloud_render_view_normals and dpe_normal_score of include/dpe_mvs.h): the kernels must give the host path's
normals, counts, sums, maps, scores and error maps bit for bit on the cases of tests/test_normal_eval.py, where the host
path is pinned to numpy references; the folder tool must give the host path's dict and table; a context must give back
what it allocated and stay usable after every refusal; the cloud calls that share its buffers must give the bits they
gave before; and a pipeline run must launch none of these kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from DPE_MVS import _abi, native, pipeline, synthetic
from test_cloud_eval import PKG, cloud_case, same_bits
from test_cloud_register import IDENTITY, STEP_R, step_clouds, sums_vector
from test_depth_eval import TAUS, render_case, score_case as depth_score_case
from test_depth_eval import same_score as same_depth_score
from test_normal_eval import (FOLDER_R, FOLDER_TAUS, NORMALS_CASES, RENDER_NORMALS_CASES, SCORE_CASES, cos_taus, normal_folder,
                              normals_case, render_normals_case, same_score, scene, score_case, sums_of)

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------ 1. device normals against host normals
@pytest.mark.parametrize("name", NORMALS_CASES)
def test_device_normals_match_host(ctx, name):
    P, R, min_nb, sums, want, _, _ = normals_case(name)
    host, host_counts, host_sums = pipeline.estimate_normals(P, R, min_nb, want_sums=True)
    assert np.array_equal(host_sums, sums) and same_bits(host, want)       # the host path is numpy's
    got, counts, got_sums = ctx.cloud_normals(P, R, min_nb, want_sums=True)
    assert np.array_equal(counts, host_counts) and np.array_equal(got_sums, host_sums), name   # the integers first
    assert same_bits(got, host), (name, int((got.view(U) != host.view(U)).any(axis=1).sum()))
    again, counts2 = ctx.cloud_normals(P, R, min_nb)                       # a second call, without the sums: the same bits
    assert same_bits(again, got) and np.array_equal(counts2, counts)


def test_device_normals_of_the_scene_and_no_points(ctx):
    sc, pts, nrm, counts = scene()
    got, got_counts = ctx.cloud_normals(pts, 0.07)
    assert same_bits(got, nrm) and np.array_equal(got_counts, counts)
    empty, none = ctx.cloud_normals(np.empty((0, 3), F), 0.1)
    assert empty.shape == (0, 3) and none.shape == (0,)
    nan, cnt, sums = ctx.cloud_normals(np.full((5, 3), np.nan, F), 0.1, want_sums=True)
    assert not nan.any() and not cnt.any() and not sums.any()


# ------------------------------------------------------------------------------ 2. device render against host render
@pytest.mark.parametrize("name", RENDER_NORMALS_CASES)
def test_device_render_with_normals_matches_host(ctx, name):
    pts, nrm, cam, s, want_depth, want_normal, _ = render_normals_case(name)
    host_depth, host_normal = pipeline.render_cloud_normals(pts, nrm, cam, s)
    assert same_bits(host_depth, want_depth) and same_bits(host_normal, want_normal)   # the host path is numpy's
    ctx.cloud_render_stage(pts, nrm)
    depth, normal = ctx.cloud_render_view_normals(cam, s)
    assert same_bits(depth, host_depth) and same_bits(normal, host_normal), name
    assert same_bits(ctx.cloud_render_view(cam, s), depth)                 # the plain render on a staging with normals, as before
    d2, n2 = ctx.cloud_render_view_normals(cam, s)                         # a second call: the same bits
    assert same_bits(d2, depth) and same_bits(n2, normal)


def test_device_pipeline_end_to_end(ctx):
    """estimate, stage, render and score on the device: the host's dict, and the issue's condition on the scene"""
    sc, pts, nrm, _ = scene()
    cam, truth = sc["cams"][0], sc["views"][0]["normals"].astype(F)
    host = pipeline.score_normals(truth, pipeline.render_cloud_normals(pts, nrm, cam, 0)[1], taus_deg=[11.25, 30.0])
    got_nrm, _ = ctx.cloud_normals(pts, 0.07)
    ctx.cloud_render_stage(pts, got_nrm)
    ctx.cloud_render_view_normals(cam, 0, download=False)
    got = ctx.normal_score(truth, None, [pipeline.normal_cos(11.25), pipeline.normal_cos(30.0)])
    assert same_score(got, host)
    assert got["n_both"] > 0.99 * got["n_px"] and got["within"][0] > 0.95 * got["n_both"]
    d = ctx.depth_score(sc["views"][0]["depth"].astype(F), None, [0.01], True)
    assert same_depth_score(d, pipeline.score_depth(sc["views"][0]["depth"].astype(F), pipeline.render_cloud(pts, cam, 0), [0.01], True))   # the depth map is resident beside the normal map


# ------------------------------------------------------------------------------ 3. device score against host score
@pytest.mark.parametrize("name", SCORE_CASES)
def test_device_score_matches_host(ctx, name):
    est, gt, want, want_err = score_case(name)
    host, host_err = pipeline.score_normals(est, gt, cos_taus=cos_taus(), want_error=True)
    assert same_score(host, want) and same_bits(host_err, want_err)        # the host path is numpy's
    got, err = ctx.normal_score(est, gt, cos_taus(), want_error=True)
    assert same_score(got, host), (name, got, host)
    assert same_bits(err, host_err)
    assert same_score(ctx.normal_score(est, gt, cos_taus()), host)         # without the error map, a second call
    assert sum(got["hist"]) == got["n_both"]
    if name.startswith("invalid"):
        assert same_bits(sums_of(got), np.zeros(2))                        # +0.0, not -0.0


@pytest.mark.parametrize("name", ["scatter-65-33-1-4097", "special-1", "scatter-1-1-0-65", "empty"])
def test_device_score_against_the_rendered_map(ctx, name):
    pts, nrm, cam, s, _, want, _ = render_normals_case(name)
    rng = np.random.default_rng(6)
    est = (want + 0.2 * rng.standard_normal(want.shape)).astype(F)
    est[rng.random(want.shape[:2]) < 0.1] = np.nan
    host, host_err = pipeline.score_normals(est, want, cos_taus=cos_taus(), want_error=True)
    ctx.cloud_render_stage(pts, nrm)
    ctx.cloud_render_view_normals(cam, s, download=False)
    got, err = ctx.normal_score(est, None, cos_taus(), want_error=True)
    assert same_score(got, host) and same_bits(err, host_err)
    with pytest.raises(native.DpeError, match="size differs"):
        ctx.normal_score(np.ones((want.shape[0] + 1, want.shape[1], 3), F), None, cos_taus())
    assert same_score(ctx.normal_score(est, None, cos_taus()), host)       # the refusal left the map


def test_depth_and_normal_scores_share_their_buffers(ctx):
    """dpe_depth_score and dpe_normal_score upload into one set of buffers: taken in turn against the resident maps of
    one view, with a normal score of another size and an explicit gt in between, each gives the host's bits"""
    pts, nrm, cam, s, want_depth, want_normal, _ = render_normals_case("scatter-65-33-1-4097")
    rng = np.random.default_rng(8)
    d_est = (want_depth * (1 + 0.05 * rng.standard_normal(want_depth.shape))).astype(F)
    d_est[rng.random(want_depth.shape) < 0.1] = np.nan
    n_est = (want_normal + 0.2 * rng.standard_normal(want_normal.shape)).astype(F)
    n_est[rng.random(want_normal.shape[:2]) < 0.1] = np.nan
    host_d, host_d_err = pipeline.score_depth(d_est, want_depth, TAUS, want_error=True)
    host_n, host_n_err = pipeline.score_normals(n_est, want_normal, cos_taus=cos_taus(), want_error=True)
    o_est, o_gt, _, _ = score_case("mixed-257-1")
    host_o, host_o_err = pipeline.score_normals(o_est, o_gt, cos_taus=cos_taus(), want_error=True)
    assert host_d["n_both"] > 0 and host_n["n_both"] > 0
    ctx.cloud_render_stage(pts, nrm)
    ctx.cloud_render_view_normals(cam, s, download=False)

    def depth():
        got, err = ctx.depth_score(d_est, None, TAUS, want_error=True)
        assert same_depth_score(got, host_d) and same_bits(err, host_d_err)

    def normal():
        got, err = ctx.normal_score(n_est, None, cos_taus(), want_error=True)
        assert same_score(got, host_n) and same_bits(err, host_n_err)

    depth()
    normal()
    got, err = ctx.normal_score(o_est, o_gt, cos_taus(), want_error=True)  # 257 x 1: the buffers at another size
    assert same_score(got, host_o) and same_bits(err, host_o_err)
    depth()
    normal()


# ------------------------------------------------------------------------------ 4. surfaces on the device
def test_folder_tool_on_the_device(tmp_path):
    d, ply, maps, sc = normal_folder(tmp_path)
    pts = pipeline.read_point_cloud(ply)
    live = native.live_device_bytes()
    for kw in ({}, dict(splat=1, min_neighbours=5), dict(gt_normals=maps), dict(write_maps=True)):
        scan, radius = (None, None) if "gt_normals" in kw else (pts, FOLDER_R)
        want = pipeline.evaluate_normal_maps(d, scan, radius, FOLDER_TAUS, **kw)
        kept = {n: open(os.path.join(d, pipeline.OUT_NAME, "00000001", n), "rb").read() for n in ("normal_gt.npy", "normal_error.npy")} if kw.get("write_maps") else {}
        assert pipeline.evaluate_normal_maps(d, scan, radius, FOLDER_TAUS, gpu_index=0, **kw) == want
        for n, data in kept.items():                                       # --maps writes the same files from the device
            assert open(os.path.join(d, pipeline.OUT_NAME, "00000001", n), "rb").read() == data
        assert native.live_device_bytes() == live                          # its own context, closed again
    outs = {}
    for flag in ("--cpu", "--gpu"):
        r = subprocess.run([os.path.join(PKG, "bin", "dpe_normal_eval"), d, ply, repr(FOLDER_R)] + [repr(t) for t in FOLDER_TAUS] +
                           ["--splat", "1", flag] + (["0"] if flag == "--gpu" else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[flag] = r.stdout
    assert outs["--gpu"] == outs["--cpu"] == pipeline.format_normal_eval(pipeline.evaluate_normal_maps(d, pts, FOLDER_R, FOLDER_TAUS, splat=1))
    cam = sc["cams"][0]
    nrm, counts = pipeline.estimate_normals(pts, FOLDER_R)
    dev_nrm, dev_counts = pipeline.estimate_normals(pts, FOLDER_R, gpu_index=0)
    assert same_bits(dev_nrm, nrm) and np.array_equal(dev_counts, counts)
    for a, b in zip(pipeline.render_cloud_normals(pts, nrm, cam, 1, gpu_index=0), pipeline.render_cloud_normals(pts, nrm, cam, 1)):
        assert same_bits(a, b)
    est, gt, want, _ = score_case("mixed-257-1")
    assert pipeline.score_normals(est, gt, cos_taus=cos_taus(), gpu_index=0) == pipeline.score_normals(est, gt, cos_taus=cos_taus())
    assert native.live_device_bytes() == live


# ------------------------------------------------------------------------------ 5. memory, refusals, neighbours
def test_states_memory_and_refusals():
    pts, nrm, cam, s, want_depth, want_normal, _ = render_normals_case("scatter-65-33-1-4097")
    est, gt, score, _ = score_case("mixed-257-1")
    P, R, min_nb, sums, normals, _, _ = normals_case("n257")
    t = cos_taus()
    live = native.live_device_bytes()
    c = native.PatchMatchContext(0)
    lib = native._LIB
    try:
        with pytest.raises(native.DpeError, match="no staged cloud"):      # a fresh context
            c.cloud_render_view_normals(cam, 0)
        with pytest.raises(native.DpeError, match="no rendered map"):
            c.normal_score(est, None, t)
        c.cloud_render_stage(pts)                                          # a staging without normals
        with pytest.raises(native.DpeError, match="no staged normals"):
            c.cloud_render_view_normals(cam, s)
        assert same_bits(c.cloud_render_view(cam, s), want_depth)           # which the refusal left usable
        with pytest.raises(native.DpeError, match="no rendered map"):      # a plain render leaves no normal map
            c.normal_score(np.ones(want_normal.shape, F), None, t)

        def still_works():
            got, counts = c.cloud_normals(P, R, min_nb)
            assert same_bits(got, normals) and np.array_equal(counts, sums[:, 0])
            c.cloud_render_stage(pts, nrm)
            depth, normal = c.cloud_render_view_normals(cam, s)
            assert same_bits(depth, want_depth) and same_bits(normal, want_normal)
            assert same_score(c.normal_score(est, gt, t), score)
        still_works()
        out_n, out_c = np.empty((len(P), 3), F), np.empty(len(P), np.int32)
        ok = (P.ctypes.data, len(P), C.c_float(R), min_nb, out_n.ctypes.data, out_c.ctypes.data, None)
        for at, v in ((0, None), (1, 2 ** 31), (2, C.c_float(0.0)), (2, C.c_float(np.nan)), (2, C.c_float(-1.0)), (3, 2), (3, 0), (4, None), (5, None)):
            args = list(ok)
            args[at] = v
            assert lib.dpe_cloud_normals(c._ctx, *args) == -1 and b"dpe_cloud_normals: bad argument" in lib.dpe_last_error(), at
        far = np.array([(0, 0, 0), (3e38, 0, 0)], F)
        with pytest.raises(native.DpeError, match="radius too small for the cloud's extent"):
            c.cloud_normals(far, 1e-30)
        still_works()
        assert lib.dpe_cloud_render_stage_normals(c._ctx, pts.ctypes.data, None, 5) == -1 and b"dpe_cloud_render_stage_normals: bad argument" in lib.dpe_last_error()
        assert lib.dpe_cloud_render_stage_normals(c._ctx, None, nrm.ctypes.data, 5) == -1
        assert lib.dpe_cloud_render_stage_normals(c._ctx, pts.ctypes.data, nrm.ctypes.data, 2 ** 31) == -1
        bad = _abi.DpeCamera()
        C.memmove(C.byref(bad), C.byref(cam), C.sizeof(bad))
        bad.width = 0
        out_d, out_m = np.empty_like(want_depth), np.empty_like(want_normal)
        for args in ((None, 0), (C.byref(bad), 0), (C.byref(cam), 9), (C.byref(cam), -1)):
            assert lib.dpe_cloud_render_view_normals(c._ctx, args[0], args[1], out_d.ctypes.data, out_m.ctypes.data) == -1
            assert b"dpe_cloud_render_view_normals: bad argument" in lib.dpe_last_error()
            depth, normal = c.cloud_render_view_normals(cam, s)             # the staging survived the refusal
            assert same_bits(depth, want_depth) and same_bits(normal, want_normal)
        sc = _abi.DpeNormalScore()
        ok = (est.ctypes.data, gt.ctypes.data, est.shape[1], est.shape[0], t.ctypes.data, 4, C.byref(sc), None)
        for at, v in ((0, None), (2, 0), (3, 0), (4, None), (5, 0), (5, 17), (6, None)):
            args = list(ok)
            args[at] = v
            assert lib.dpe_normal_score(c._ctx, *args) == -1 and b"dpe_normal_score: bad argument" in lib.dpe_last_error(), at
        for v in (-1.5, 1.5, np.nan, np.inf):
            with pytest.raises(native.DpeError, match="dpe_normal_score: bad argument"):
                c.normal_score(est, gt, [0.5, v])
        still_works()
        Q, T, Rn, nn = cloud_case("random")
        c.cloud_render_stage(pts, nrm)
        assert same_bits(c.cloud_nn(Q, T, Rn), nn)                          # another cloud call ends the staging
        with pytest.raises(native.DpeError, match="no staged cloud"):
            c.cloud_render_view_normals(cam, s)
        c.cloud_render_stage(pts, nrm)
        c.cloud_normals(P, R, min_nb)                                       # and so does dpe_cloud_normals
        with pytest.raises(native.DpeError, match="no staged cloud"):
            c.cloud_render_view_normals(cam, s)
        assert native.live_device_bytes() > live
    finally:
        c.close()
    assert native.live_device_bytes() == live                               # the context gave everything back


def test_neighbouring_cloud_calls_keep_their_bits(ctx):
    pts, nrm, cam, s, want_depth, want_normal, _ = render_normals_case("scatter-65-33-1-4097")
    P, R, min_nb, sums, normals, _, _ = normals_case("spread")
    est, gt, score, _ = score_case("mixed-257-1")
    Q, T, Rn, nn = cloud_case("random")
    cl = step_clouds()
    S = cl["third"][:4097]
    host_step = pipeline.cloud_icp_step(S, cl["G"], STEP_R, IDENTITY)
    plain = render_case("scatter-65-33-1-4097")
    d_est, d_gt, relative, d_score, _ = depth_score_case("mixed-257-1-abs")
    vox = pipeline.voxel_down_sample(P, 0.05)

    def the_new_calls():
        got, counts = ctx.cloud_normals(P, R, min_nb)
        assert same_bits(got, normals) and np.array_equal(counts, sums[:, 0])
        ctx.cloud_render_stage(pts, nrm)
        depth, normal = ctx.cloud_render_view_normals(cam, s)
        assert same_bits(depth, want_depth) and same_bits(normal, want_normal)
        assert same_score(ctx.normal_score(est, gt, cos_taus()), score)
    the_new_calls()
    assert same_bits(ctx.cloud_nn(Q, T, Rn), nn)                            # cloud_nn
    the_new_calls()
    got = ctx.cloud_voxel(P, 0.05)                                          # cloud_voxel
    assert same_bits(got[0], vox[0]) and np.array_equal(got[2], vox[2]) and np.array_equal(got[3], vox[3])
    the_new_calls()
    ctx.cloud_icp_stage(S, cl["G"], STEP_R)                                 # an ICP step, with a normal score in between
    assert same_score(ctx.normal_score(est, gt, cos_taus()), score)
    step = ctx.cloud_icp_step(IDENTITY)
    assert step["matched"] == host_step["matched"] and same_bits(sums_vector(step), sums_vector(host_step))
    the_new_calls()
    ctx.cloud_render_stage(plain[0])                                        # cloud_render_view and depth_score
    assert same_bits(ctx.cloud_render_view(plain[1], plain[2]), plain[3])
    assert same_depth_score(ctx.depth_score(d_est, d_gt, TAUS, relative), d_score)
    the_new_calls()


def test_pipeline_launches_none_of_these_kernels(tmp_path):
    d = str(tmp_path / "dense")
    synthetic.write_dense_folder(d, 64, 48, 4)
    before = native.cloud_launches()
    assert pipeline.run_dpe_pipeline(d, verbose=False, normal=True) == 0
    assert native.cloud_launches() == before
    # and the normal maps it wrote are what the tool scores
    pts = synthetic.gt_point_cloud(synthetic.make_scene(64, 48, 4), 1)
    e = pipeline.evaluate_normal_maps(d, pts, 0.1, [11.25, 30.0], gpu_index=0)
    assert e == pipeline.evaluate_normal_maps(d, pts, 0.1, [11.25, 30.0])
    assert len(e["images"]) == 4 and e["total"]["n_both"] > 0
    print("normal.npy of a pipeline run: within 30 degrees", e["total"]["share"][1], "median", e["total"]["median_deg"])
    assert native.cloud_launches() > before
