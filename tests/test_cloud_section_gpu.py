"""The bookkeeping of the cloud section (csrc/dpe_cloud.hip): every kernel launch is counted once, whatever call makes
it, and dpe_cloud_last_timings keeps the slot meanings include/dpe_mvs.h states.  What the calls compute is held to the
host path by tests/test_cloud_*_gpu.py, tests/test_depth_eval_gpu.py and tests/test_normal_eval_gpu.py."""
import math

import numpy as np
import pytest

from DPE_MVS import native
from test_depth_eval import pixel_camera

pytestmark = pytest.mark.gpu
F = np.float32
R = 0.2                                                                 # a radius and a voxel the unit cube admits
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
SLOTS = ("stage", "build", "query", "download")


def cube(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(F)


def scan(n, w, h):
    """n points in front of pixel_camera(w, h), inside the image"""
    p = cube(n, 3)
    z = F(2.0)
    return np.stack([p[:, 0] * F(w - 1) * z, p[:, 1] * F(h - 1) * z, np.full(n, z, F)], -1).astype(F)


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.set_timing(False)
    c.close()


def launches(call):
    before = native.cloud_launches()
    call()
    return native.cloud_launches() - before


def test_launch_counts_per_call(ctx):
    A, B = cube(300, 1), cube(400, 2)
    nowhere = np.full((5, 3), np.nan, F)
    assert launches(lambda: ctx.cloud_nn(A, B, R)) == 9                  # 2 bounds, 2 x 3 build, 1 query
    assert launches(lambda: ctx.cloud_nn_index(A, B, R)) == 9
    assert launches(lambda: ctx.cloud_nn_pair(A, B, R)) == 16            # 2 bounds, 2 x (2 x 3 build + 1 query)
    assert launches(lambda: ctx.cloud_nn(A, nowhere, R)) == 2            # the bounds alone
    assert launches(lambda: ctx.cloud_voxel(A, R)) == 7                  # bounds, cells, insert, mark, count, scan, fill
    assert launches(lambda: ctx.cloud_icp_stage(A, B, R)) == 5           # 2 bounds, 3 build
    for n, want in ((256, 6), (257, 7), (65537, 8)):                     # apply, 3 build, match, terms, then the tree's levels
        ctx.cloud_icp_stage(cube(n, 4), B, R)
        assert launches(lambda: ctx.cloud_icp_step(IDENTITY)) == want, n
    cam = pixel_camera(33, 17)
    assert launches(lambda: ctx.cloud_render_stage(scan(300, 33, 17))) == 0
    assert launches(lambda: ctx.cloud_render_view(cam, 1)) == 3          # clear, splat, finish
    ctx.cloud_render_stage(np.empty((0, 3), F))
    assert launches(lambda: ctx.cloud_render_view(cam, 1)) == 2          # an empty scan: no splat
    for (w, h), want in (((16, 16), 1), ((17, 16), 2), ((257, 256), 3)):
        est = np.ones((h, w), F)
        assert launches(lambda: ctx.depth_score(est, est, [0.1])) == want, (w, h)
        nrm = np.ones((h, w, 3), F)
        assert launches(lambda: ctx.normal_score(nrm, nrm, [0.5])) == want, (w, h)
    assert launches(lambda: ctx.cloud_normals(A, R)) == 5                # bounds, 3 build, normal
    assert launches(lambda: ctx.cloud_normals(nowhere, R)) == 1          # the bounds alone
    pts = scan(300, 33, 17)
    assert launches(lambda: ctx.cloud_render_stage(pts, np.ones_like(pts))) == 0
    assert launches(lambda: ctx.cloud_render_view_normals(cam, 1)) == 4  # clear, splat, finish, normals
    ctx.cloud_render_stage(np.empty((0, 3), F), np.empty((0, 3), F))
    assert launches(lambda: ctx.cloud_render_view_normals(cam, 1)) == 3  # an empty scan: no splat


def test_timings_contract(ctx):
    A, B = cube(300, 1), cube(400, 2)
    cam = pixel_camera(33, 17)
    est = np.ones((17, 33), F)
    ctx.set_timing(False)
    ctx.cloud_nn(A, B, R)
    assert ctx.cloud_timings() == {}
    ctx.set_timing(True)

    def timed(call, zero=()):
        call()
        t = ctx.cloud_timings()
        assert tuple(t) == SLOTS, t
        assert all(math.isfinite(v) and v >= 0.0 for v in t.values()), t
        for k in zero:
            assert t[SLOTS[k]] == 0.0, (k, t)

    timed(lambda: ctx.cloud_nn(A, B, R))
    timed(lambda: ctx.cloud_nn_pair(A, B, R))
    timed(lambda: ctx.cloud_nn_index(A, B, R))
    timed(lambda: ctx.cloud_voxel(A, R))
    ctx.cloud_icp_stage(A, B, R)
    timed(lambda: ctx.cloud_icp_step(IDENTITY))
    timed(lambda: ctx.cloud_render_stage(scan(300, 33, 17)), zero=(1, 2, 3))
    timed(lambda: ctx.cloud_render_view(cam, 1), zero=(0, 2))
    timed(lambda: ctx.depth_score(est, None, [0.1]), zero=(1,))
    timed(lambda: ctx.cloud_normals(A, R))
    pts = scan(300, 33, 17)
    timed(lambda: ctx.cloud_render_stage(pts, np.ones_like(pts)), zero=(1, 2, 3))
    timed(lambda: ctx.cloud_render_view_normals(cam, 1), zero=(0, 2))
    timed(lambda: ctx.normal_score(np.ones((17, 33, 3), F), None, [0.5]), zero=(1,))
    for none in (np.empty((0, 3), F), np.full((5, 3), np.nan, F)):       # no points, or none finite: nothing is timed
        ctx.cloud_normals(none, R)
        assert ctx.cloud_timings() == {}
    ctx.cloud_icp_stage(A, np.empty((0, 3), F), R)                       # nothing to match: the step launches and times nothing
    assert ctx.cloud_icp_step(IDENTITY)["matched"] == 0
    assert ctx.cloud_timings() == {}
