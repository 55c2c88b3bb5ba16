"""Rigid registration on the device (csrc/pass_register.h; dpe_cloud_nn_index, dpe_cloud_icp_stage and
dpe_cloud_icp_step of include/dpe_mvs.h): the kernels must give the host path's indices, distances and 16 sums bit for
bit on the clouds of tests/test_cloud_register.py, where the host path is pinned to numpy references; the loop, the
evaluation and the command lines must give the host path's structs, tables and files; a context must give back what it
allocated and stay usable after every refusal; and a pipeline run must launch none of these kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from DPE_MVS import native, pipeline, synthetic
from test_cloud_eval import CLOUDS, PKG, cloud_case, same_bits
from test_cloud_register import (IDENTITY, INDEX_CLOUDS, REGISTER, STEP_R, T_ROT, index_case, motion_case, register_flags, registered_files,
                                 step_clouds, sums_vector)
from test_cloud_voxel import write_ply
from voxel_clouds import voxel_case

pytestmark = pytest.mark.gpu
F = np.float32
GPU_STEP_SIZES = [1, 3, 63, 64, 65, 255, 256, 257, 4097, 65537]


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------ 1. device index against host index
@pytest.mark.parametrize("name", sorted(INDEX_CLOUDS))
def test_device_index_matches_host(ctx, name):
    Q, T, R, want_d2, want_idx = index_case(name)
    plain = ctx.cloud_nn(Q, T, R)
    d2, idx = ctx.cloud_nn_index(Q, T, R)
    h_d2, h_idx = pipeline.cloud_nn_index(Q, T, R)
    assert np.array_equal(idx, h_idx) and same_bits(d2, h_d2)
    assert np.array_equal(idx, want_idx) and same_bits(d2, want_d2)        # and numpy's
    d2b, idxb = ctx.cloud_nn_index(Q, T, R)                                # a second run: the same arrays
    assert same_bits(d2b, d2) and same_bits(idxb, idx)
    assert same_bits(ctx.cloud_nn(Q, T, R), plain) and same_bits(plain, d2)   # cloud_nn gives the bits it gave before
    if name in CLOUDS:
        assert same_bits(plain, cloud_case(name)[3])


# ------------------------------------------------------------------------------ 2. device step against host step
def host_step(P, G, T):
    return pipeline.cloud_icp_step(P, G, STEP_R, T)


@pytest.mark.parametrize("kind,T", [("third", IDENTITY), ("third", T_ROT), ("far", IDENTITY), ("nonfinite", T_ROT)],
                         ids=["identity", "rotated", "all_unmatched", "nonfinite"])
def test_device_step_matches_host(ctx, kind, T):
    c = step_clouds()
    for n in GPU_STEP_SIZES:
        P = c[kind][:n]
        want = host_step(P, c["G"], T)
        ctx.cloud_icp_stage(P, c["G"], STEP_R)
        got = ctx.cloud_icp_step(T)
        assert got["matched"] == want["matched"], n
        assert same_bits(sums_vector(got), sums_vector(want)), (n, sums_vector(got) - sums_vector(want))
        if kind == "far":
            assert got["matched"] == 0 and same_bits(sums_vector(got), np.zeros(16))       # +0.0, not -0.0
    if kind == "third":
        assert want["matched"] > 40000


def test_two_steps_over_one_staging_and_a_step_without_one(ctx):
    c = step_clouds()
    P = c["third"][:4097]
    ctx.cloud_icp_stage(P, c["G"], STEP_R)
    for T in (IDENTITY, T_ROT, IDENTITY):
        got, want = ctx.cloud_icp_step(T), host_step(P, c["G"], T)
        assert got["matched"] == want["matched"] and same_bits(sums_vector(got), sums_vector(want))
    ctx.cloud_icp_stage(P, np.empty((0, 3), F), STEP_R)                    # an empty target: staged, nothing matches
    got = ctx.cloud_icp_step(IDENTITY)
    assert got["matched"] == 0 and same_bits(sums_vector(got), np.zeros(16))
    ctx.cloud_nn(P, c["G"], STEP_R)                                        # another cloud call ends the staging
    with pytest.raises(native.DpeError, match="no staged pair"):
        ctx.cloud_icp_step(IDENTITY)
    fresh = native.PatchMatchContext(0)
    try:
        with pytest.raises(native.DpeError, match="no staged pair"):
            fresh.cloud_icp_step(IDENTITY)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------ 3. the loop on the device
@pytest.mark.parametrize("radii", [[0.15], [0.3, 0.05]], ids=["one_stage", "two_stages"])
def test_loop_on_the_device(radii):
    P, G, _ = motion_case()
    host = pipeline.register_clouds(P, G, radii, max_iters=50)
    dev = pipeline.register_clouds(P, G, radii, max_iters=50, gpu_index=0)
    assert same_bits(np.array(dev["T"]), np.array(host["T"]))
    assert dev == host                                                      # iters, matched, rms and converged as well
    assert [s["converged"] for s in dev["stages"]] == [2] * len(radii) and dev["stages"][-1]["matched"] == 1500


# ------------------------------------------------------------------------------ 4. surfaces on the device
def test_surfaces_on_the_device(tmp_path):
    recon, gt, taus, v, lo, hi, moved, T, want = registered_files(tmp_path)
    live = native.live_device_bytes()
    assert pipeline.evaluate_clouds(moved, T, taus, voxel=v, crop=(lo, hi), register=REGISTER, gpu_index=0) == want
    assert native.live_device_bytes() == live                              # its own context, closed again
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_eval"), recon, gt] + [repr(t) for t in taus] +
                       ["--voxel", repr(v), "--crop"] + [repr(x) for x in lo + hi] + ["--gpu", "0"] + register_flags(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == pipeline.format_cloud_eval(want)
    P, G, _ = motion_case()
    col = np.random.default_rng(8).integers(0, 256, P.shape).astype(np.uint8)
    write_ply(tmp_path / "src.ply", P, col)
    write_ply(tmp_path / "tgt.ply", G)
    outs = {}
    for flag in ("--cpu", "--gpu"):
        out = str(tmp_path / (flag[2:] + ".ply"))
        r = subprocess.run([os.path.join(PKG, "bin", "dpe_register"), str(tmp_path / "src.ply"), str(tmp_path / "tgt.ply"), out, "0.3", "0.05", flag] +
                           (["0"] if flag == "--gpu" else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[flag] = (r.stdout, open(out, "rb").read())
    assert outs["--gpu"] == outs["--cpu"]


# ------------------------------------------------------------------------------ 5. memory and idle runs
def test_memory_and_refusals():
    P, G, _ = motion_case()
    want = pipeline.register_clouds(P, G, 0.15)
    live = native.live_device_bytes()
    c = native.PatchMatchContext(0)
    lib = native._LIB

    def still_works():
        c.cloud_icp_stage(P, G, 0.15)
        host = pipeline.cloud_icp_step(P, G, 0.15, IDENTITY)
        got = c.cloud_icp_step(IDENTITY)
        assert got["matched"] == host["matched"] and same_bits(sums_vector(got), sums_vector(host))
        Q, T, R, nn = cloud_case("random")
        assert same_bits(c.cloud_nn(Q, T, R), nn)
        V, v, Cc, _, col = voxel_case("random")
        assert all(same_bits(a, b) for a, b in zip(c.cloud_voxel(V, v, Cc), col[:4]))
    try:
        still_works()
        s = pipeline.DpeIcpSums()
        for args in ((None, len(P), G.ctypes.data, len(G), 0.15), (P.ctypes.data, len(P), None, len(G), 0.15),
                     (P.ctypes.data, 2 ** 31, G.ctypes.data, len(G), 0.15), (P.ctypes.data, len(P), G.ctypes.data, len(G), 0.0),
                     (P.ctypes.data, len(P), G.ctypes.data, len(G), float("nan")), (P.ctypes.data, len(P), G.ctypes.data, len(G), float("inf"))):
            assert lib.dpe_cloud_icp_stage(c._ctx, *args) == -1 and b"dpe_cloud_icp_stage: bad argument" in lib.dpe_last_error()
            still_works()
        c.cloud_icp_stage(P + F(50), G, 0.15)                               # what the loop refuses as "fewer than 3 matches"
        assert c.cloud_icp_step(IDENTITY)["matched"] == 0
        still_works()
        far = np.array([[-1e30, 0, 0], [1e30, 0, 0]], F)
        with pytest.raises(native.DpeError, match="radius too small for the cloud's extent"):
            c.cloud_icp_stage(P, far, 1e-3)
        with pytest.raises(native.DpeError, match="no staged pair"):        # a failed staging leaves none
            c.cloud_icp_step(IDENTITY)
        still_works()
        c.cloud_icp_stage(P, G, 0.15)
        assert lib.dpe_cloud_icp_step(c._ctx, None, C.byref(s)) == -1 and lib.dpe_cloud_icp_step(c._ctx, IDENTITY.ctypes.data, None) == -1
        with pytest.raises(native.DpeError, match="dpe_cloud_nn_index: bad argument"):
            c.cloud_nn_index(P, G, 0.0)
        still_works()
        assert native.live_device_bytes() > live
    finally:
        c.close()
    assert native.live_device_bytes() == live                              # the context gave everything back
    # the loop's refusals through a context of their own, then the same process still registers
    for kw, message in ((dict(radii=[0.15], src=P + F(50)), "fewer than 3 matches"), (dict(radii=[0.0]), "radius is not a finite positive"),
                        (dict(radii=[0.15], max_iters=0), "1 to 1000 iterations"), (dict(radii=[1e-3], tgt=far), "radius too small")):
        with pytest.raises(pipeline.PipelineError, match=message):
            pipeline.register_clouds(kw.pop("src", P), kw.pop("tgt", G), gpu_index=0, **kw)
        assert native.live_device_bytes() == live
    assert pipeline.register_clouds(P, G, 0.15, gpu_index=0) == want


def test_pipeline_launches_none_of_these_kernels(tmp_path):
    d = str(tmp_path / "dense")
    synthetic.write_dense_folder(d, 64, 48, 4)
    before = native.cloud_launches()
    assert pipeline.run_dpe_pipeline(d, verbose=False, fusion=True) == 0
    assert native.cloud_launches() == before
    P, G, _ = motion_case()
    pipeline.register_clouds(P, G, 0.15, gpu_index=0)
    assert native.cloud_launches() > before
