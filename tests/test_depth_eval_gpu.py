"""Depth-map evaluation on the device (csrc/pass_render.h; dpe_cloud_render_stage, dpe_cloud_render_view and
dpe_depth_score of include/dpe_mvs.h): the kernels must give the host path's maps, counts, sums and error maps bit for
bit on the cases of tests/test_depth_eval.py, where the host path is pinned to numpy references; the folder tool must
give the host path's dict and table; a context must give back what it allocated and stay usable after every refusal;
the cloud calls that share its buffers must give the bits they gave before; and a pipeline run must launch none of these
kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from DPE_MVS import _abi, native, pipeline, synthetic
from test_cloud_eval import PKG, cloud_case, same_bits
from test_cloud_register import IDENTITY, STEP_R, step_clouds, sums_vector
from test_depth_eval import (FOLDER_TAUS, RENDER_CASES, SCORE_CASES, TAUS, depth_folder, render_case, rotated_camera, same_score,
                             score_case, sums_of)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------ 1. device render against host render
@pytest.mark.parametrize("name", RENDER_CASES)
def test_device_render_matches_host(ctx, name):
    pts, cam, s, want = render_case(name)
    host = pipeline.render_cloud(pts, cam, s)
    assert same_bits(host, want)                                          # the host path is numpy's
    ctx.cloud_render_stage(pts)
    got = ctx.cloud_render_view(cam, s)
    assert same_bits(got, host), (name, int((got.view(np.uint32) != host.view(np.uint32)).sum()))
    assert same_bits(ctx.cloud_render_view(cam, s), got)                  # a second call: the same bits


def test_three_cameras_over_one_staging_and_a_view_without_one(ctx):
    pts = render_case("scatter-65-33-1-4097")[0]
    ctx.cloud_render_stage(pts)
    for (w, h, s) in ((65, 33, 1), (7, 5, 2), (96, 72, 0)):
        cam = rotated_camera(w, h, 1000.0)[0]
        got = ctx.cloud_render_view(cam, s)
        assert same_bits(got, pipeline.render_cloud(pts, cam, s))
        assert got.any()
    Q, T, R, nn = cloud_case("random")
    assert same_bits(ctx.cloud_nn(Q, T, R), nn)                           # another cloud call ends the staging
    with pytest.raises(native.DpeError, match="no staged cloud"):
        ctx.cloud_render_view(cam, 0)
    fresh = native.PatchMatchContext(0)
    try:
        with pytest.raises(native.DpeError, match="no staged cloud"):
            fresh.cloud_render_view(cam, 0)
        with pytest.raises(native.DpeError, match="no rendered map"):
            fresh.depth_score(np.ones((5, 7), F), None, [0.1])
    finally:
        fresh.close()


# ------------------------------------------------------------------------------ 2. device score against host score
@pytest.mark.parametrize("name", SCORE_CASES)
def test_device_score_matches_host(ctx, name):
    est, gt, relative, want, want_err = score_case(name)
    host, host_err = pipeline.score_depth(est, gt, TAUS, relative, want_error=True)
    assert same_score(host, want) and same_bits(host_err, want_err)       # the host path is numpy's
    got, err = ctx.depth_score(est, gt, TAUS, relative, want_error=True)
    assert same_score(got, host), (got, host)
    assert same_bits(err, host_err)
    assert same_score(ctx.depth_score(est, gt, TAUS, relative), host)     # without the error map
    if name.startswith("invalid"):
        assert same_bits(sums_of(got), np.zeros(3))                        # +0.0, not -0.0


@pytest.mark.parametrize("name", ["scatter-65-33-1-4097", "border-7-5-2", "scatter-1-1-0-65", "empty"])
@pytest.mark.parametrize("relative", [False, True], ids=["abs", "rel"])
def test_device_score_against_the_rendered_map(ctx, name, relative):
    pts, cam, s, want = render_case(name)
    rng = np.random.default_rng(6)
    est = (want * (1 + 0.05 * rng.standard_normal(want.shape)) + (rng.random(want.shape) < 0.1)).astype(F)
    est[rng.random(want.shape) < 0.1] = np.nan
    host, host_err = pipeline.score_depth(est, want, TAUS, relative, want_error=True)
    ctx.cloud_render_stage(pts)
    ctx.cloud_render_view(cam, s, download=False)
    got, err = ctx.depth_score(est, None, TAUS, relative, want_error=True)
    assert same_score(got, host) and same_bits(err, host_err)
    with pytest.raises(native.DpeError, match="size differs"):
        ctx.depth_score(np.ones((want.shape[0] + 1, want.shape[1]), F), None, TAUS)
    assert same_score(ctx.depth_score(est, None, TAUS, relative), host)    # the refusal left the map


# ------------------------------------------------------------------------------ 3. surfaces on the device
def test_folder_tool_on_the_device(tmp_path):
    d, ply, maps, sc = depth_folder(tmp_path)
    pts = pipeline.read_point_cloud(ply)
    live = native.live_device_bytes()
    taus = [repr(t) for t in FOLDER_TAUS]
    for kw in ({}, dict(relative=True, splat=1), dict(gt_maps=maps), dict(write_maps=True, map_name="depth_filtered.npy")):
        scan = None if "gt_maps" in kw else pts
        want = pipeline.evaluate_depth_maps(d, scan, FOLDER_TAUS, **kw)
        kept = {n: open(os.path.join(d, pipeline.OUT_NAME, "00000001", n), "rb").read() for n in ("depth_gt.npy", "depth_error.npy")} if kw.get("write_maps") else {}
        assert pipeline.evaluate_depth_maps(d, scan, FOLDER_TAUS, gpu_index=0, **kw) == want
        for n, data in kept.items():                                       # --maps writes the same files from the device
            assert open(os.path.join(d, pipeline.OUT_NAME, "00000001", n), "rb").read() == data
        assert native.live_device_bytes() == live                          # its own context, closed again
    outs = {}
    for flag in ("--cpu", "--gpu"):
        r = subprocess.run([os.path.join(PKG, "bin", "dpe_depth_eval"), d, ply] + taus + ["--relative", "--splat", "1", flag] +
                           (["0"] if flag == "--gpu" else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[flag] = r.stdout
    assert outs["--gpu"] == outs["--cpu"] == pipeline.format_depth_eval(pipeline.evaluate_depth_maps(d, pts, FOLDER_TAUS, relative=True, splat=1))
    cam = sc["cams"][0]
    assert same_bits(pipeline.render_cloud(pts, cam, 1, gpu_index=0), pipeline.render_cloud(pts, cam, 1))
    est, gt, relative, want, _ = score_case("mixed-257-1-rel")
    assert pipeline.score_depth(est, gt, TAUS, relative, gpu_index=0) == pipeline.score_depth(est, gt, TAUS, relative)
    assert native.live_device_bytes() == live


# ------------------------------------------------------------------------------ 4. memory, refusals, neighbours
def test_memory_and_refusals():
    pts, cam, s, want = render_case("scatter-65-33-1-4097")
    est, gt, relative, score, _ = score_case("mixed-257-1-abs")
    live = native.live_device_bytes()
    c = native.PatchMatchContext(0)
    lib = native._LIB

    def still_works():
        c.cloud_render_stage(pts)
        assert same_bits(c.cloud_render_view(cam, s), want)
        assert same_score(c.depth_score(est, gt, TAUS, relative), score)
    try:
        still_works()
        out = np.empty_like(want)
        t = np.array(TAUS, F)
        sc = _abi.DpeDepthScore()
        assert lib.dpe_cloud_render_stage(c._ctx, None, 5) == -1 and b"dpe_cloud_render_stage: bad argument" in lib.dpe_last_error()
        assert lib.dpe_cloud_render_stage(c._ctx, pts.ctypes.data, 2 ** 31) == -1
        still_works()
        bad = _abi.DpeCamera()
        C.memmove(C.byref(bad), C.byref(cam), C.sizeof(bad))
        bad.width = 0
        for args in ((None, 0), (C.byref(bad), 0), (C.byref(cam), 9), (C.byref(cam), -1)):
            assert lib.dpe_cloud_render_view(c._ctx, args[0], args[1], out.ctypes.data) == -1
            assert b"dpe_cloud_render_view: bad argument" in lib.dpe_last_error()
            assert same_bits(c.cloud_render_view(cam, s), want)              # the staging survived the refusal
        ok = (est.ctypes.data, gt.ctypes.data, est.shape[1], est.shape[0], t.ctypes.data, 4, 0, C.byref(sc), None)
        for at, v in ((0, None), (2, 0), (3, 0), (4, None), (5, 0), (5, 17), (6, 2), (7, None)):
            args = list(ok)
            args[at] = v
            assert lib.dpe_depth_score(c._ctx, *args) == -1 and b"dpe_depth_score: bad argument" in lib.dpe_last_error(), at
        for v in (-0.5, np.nan, np.inf):
            with pytest.raises(native.DpeError, match="dpe_depth_score: bad argument"):
                c.depth_score(est, gt, [0.1, v])
        still_works()
        assert native.live_device_bytes() > live
    finally:
        c.close()
    assert native.live_device_bytes() == live                               # the context gave everything back


def test_neighbouring_cloud_calls_keep_their_bits(ctx):
    pts, cam, s, want = render_case("scatter-65-33-1-4097")
    Q, T, R, nn = cloud_case("random")
    cl = step_clouds()
    P = cl["third"][:4097]
    host = pipeline.cloud_icp_step(P, cl["G"], STEP_R, IDENTITY)
    ctx.cloud_icp_stage(P, cl["G"], STEP_R)
    ctx.cloud_render_stage(pts)                                             # ends the staged pair: it overwrites the source
    with pytest.raises(native.DpeError, match="no staged pair"):
        ctx.cloud_icp_step(IDENTITY)
    assert same_bits(ctx.cloud_render_view(cam, s), want)
    assert same_bits(ctx.cloud_nn(Q, T, R), nn)
    ctx.cloud_icp_stage(P, cl["G"], STEP_R)
    est, gt, relative, score, _ = score_case("mixed-257-1-abs")
    assert same_score(ctx.depth_score(est, gt, TAUS, relative), score)      # a score between stage and step disturbs neither
    got = ctx.cloud_icp_step(IDENTITY)
    assert got["matched"] == host["matched"] and same_bits(sums_vector(got), sums_vector(host))


def test_pipeline_launches_none_of_these_kernels(tmp_path):
    d = str(tmp_path / "dense")
    synthetic.write_dense_folder(d, 64, 48, 4)
    before = native.cloud_launches()
    assert pipeline.run_dpe_pipeline(d, verbose=False) == 0
    assert native.cloud_launches() == before
    # and the maps it wrote are what the tool scores
    pts = synthetic.gt_point_cloud(synthetic.make_scene(64, 48, 4), 1)
    e = pipeline.evaluate_depth_maps(d, pts, [0.05], relative=True, gpu_index=0)
    assert e == pipeline.evaluate_depth_maps(d, pts, [0.05], relative=True)
    assert len(e["images"]) == 4 and e["total"]["n_both"] > 0
    assert native.cloud_launches() > before
