"""Voxel down-sampling on the device (csrc/pass_voxel.h, dpe_cloud_voxel of include/dpe_mvs.h): the kernels must give
the host path's records bit for bit (xyz, rgb, first, count) on every cloud of tests/voxel_clouds.py, where
tests/test_cloud_voxel.py pins the host path to a numpy reference, the same bits on every run, the host path's dict
and files through evaluate_clouds, bin/dpe_eval and bin/dpe_voxel, and a pipeline run must launch none of them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from DPE_MVS import native, pipeline, synthetic
from test_cloud_eval import PKG, cloud_case, same_bits
from test_cloud_voxel import check_against, prepared_files, write_ply
from voxel_clouds import CASES, F, voxel_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------ 1. device against host
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matches_host(ctx, name):
    P, v, Cc, plain, col = voxel_case(name)
    got = ctx.cloud_voxel(P, v)
    check_against(got, pipeline.voxel_down_sample(P, v), name)
    check_against(got, plain, name)
    got = ctx.cloud_voxel(P, v, Cc)
    check_against(got, pipeline.voxel_down_sample(P, v, Cc), name + " with colours")
    check_against(got, col, name + " with colours")
    check_against(ctx.cloud_voxel(P, v, Cc), got, name + ", second run")   # two device runs: equal bits


@pytest.mark.parametrize("name", ["empty", "one", "all_nan"])
def test_degenerate_inputs(ctx, name):
    P, v, Cc, plain, col = voxel_case(name)
    before = native.cloud_launches()
    xyz, rgb, first, count = ctx.cloud_voxel(P, v, Cc)
    assert len(xyz) == len(rgb) == len(first) == len(count) == (1 if name == "one" else 0)
    if name == "empty":
        assert native.cloud_launches() == before                           # nothing to do: nothing launched
    if name == "all_nan":
        assert native.cloud_launches() == before + 1                       # the staging's bounds and nothing else
    if name == "one":
        assert first.tolist() == [0] and count.tolist() == [1] and same_bits(rgb, Cc)
        assert (np.abs(xyz.view(np.int32) - P.view(np.int32)) <= 1).all()  # the point, within one float ulp


# ------------------------------------------------------------------------------ 2. errors, memory
def test_argument_errors_and_memory():
    live = native.live_device_bytes()
    c = native.PatchMatchContext(0)
    try:
        P, v, Cc, plain, col = voxel_case("random")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(native.DpeError, match=r"\(-1\).*dpe_cloud_voxel: bad argument"):   # DPE_ERR_ARG
                c.cloud_voxel(P, bad)
        far = np.array([[-1e30, 0, 0], [1e30, 0, 0]], F)
        with pytest.raises(native.DpeError, match=r"\(-1\).*voxel too small for the cloud's extent"):
            c.cloud_voxel(far, 1e-3)
        lib = native._LIB
        k_want = len(plain[2])
        xyz, first, count = np.full((k_want, 3), 7.5, F), np.full(k_want, -7, np.int32), np.full(k_want, -7, np.int32)
        k = C.c_size_t(12345)
        args = (P.ctypes.data, len(P), None, float(v), xyz.ctypes.data, None, first.ctypes.data, count.ctypes.data)
        assert lib.dpe_cloud_voxel(c._ctx, *args, k_want - 1, C.byref(k)) == -1                    # cap too small
        assert k.value == k_want and b"too small" in lib.dpe_last_error()
        assert (xyz == 7.5).all() and (first == -7).all() and (count == -7).all()                # nothing written
        assert lib.dpe_cloud_voxel(c._ctx, *args, k_want, None) == -1
        assert lib.dpe_cloud_voxel(c._ctx, None, len(P), None, float(v), *args[4:], k_want, C.byref(k)) == -1
        assert lib.dpe_cloud_voxel(c._ctx, P.ctypes.data, 2 ** 31, *args[2:], k_want, C.byref(k)) == -1
        assert lib.dpe_cloud_voxel(None, *args, k_want, C.byref(k)) == -1
        check_against(c.cloud_voxel(P, v, Cc), col, "after the refusals")                         # still usable
        Q, T, R, want = cloud_case("random")
        assert same_bits(c.cloud_nn(Q, T, R), want)                                               # and so are the distances
        assert native.live_device_bytes() > live
    finally:
        c.close()
    assert native.live_device_bytes() == live                              # the context gave everything back


# ------------------------------------------------------------------------------ 3. the evaluation and the command lines
def test_evaluate_and_command_lines_on_the_device(tmp_path):
    recon, gt, taus, v, lo, hi, want = prepared_files(tmp_path)
    Q, T, _, _ = cloud_case("line")
    live = native.live_device_bytes()
    assert pipeline.evaluate_clouds(Q, T, taus, voxel=v, crop=(lo, hi), gpu_index=0) == want
    assert pipeline.evaluate_clouds(Q, T, taus, voxel=v, gpu_index=0) == pipeline.evaluate_clouds(Q, T, taus, voxel=v)
    assert native.live_device_bytes() == live                              # its own context, closed again
    with pytest.raises(pipeline.PipelineError, match="voxel too small for the cloud's extent"):
        pipeline.evaluate_clouds(Q, np.array([[-1e30, 0, 0], [1e30, 0, 0]], F), [1e-3], voxel=1e-3, gpu_index=0)
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_eval"), recon, gt] + [repr(t) for t in taus] +
                       ["--voxel", repr(v), "--crop"] + [repr(x) for x in lo + hi] + ["--gpu", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == pipeline.format_cloud_eval(want)
    P, v, Cc, _, col = voxel_case("adversarial_R")
    write_ply(tmp_path / "in.ply", P, Cc)
    for flag, out in (("--cpu", "c.ply"), ("--gpu", "g.ply")):
        r = subprocess.run([os.path.join(PKG, "bin", "dpe_voxel"), str(tmp_path / "in.ply"), str(tmp_path / out), repr(float(v)), flag] +
                           (["0"] if flag == "--gpu" else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert open(tmp_path / "g.ply", "rb").read() == open(tmp_path / "c.ply", "rb").read()
    xyz, bgr = pipeline.read_point_cloud_colors(str(tmp_path / "g.ply"))
    assert same_bits(xyz, col[0]) and same_bits(bgr, col[1])
    assert all(same_bits(a, b) for a, b in zip(pipeline.voxel_down_sample(P, v, Cc, gpu_index=0), col[:4]))


# ------------------------------------------------------------------------------ 4. the pipeline, end to end
def test_fused_cloud_scored_after_down_sampling(tmp_path):
    """The 64 x 48, 4-view synthetic dense folder through the pipeline with fusion (which launches no kernel of this
    section), then DPE/DPE.ply against synthetic.gt_point_cloud at tau = 1, 2, 4, 8 pixel footprints with both clouds
    down-sampled at voxel = tau_max / 2.  No F-score is fixed: the device must give the host dict, the preparation
    must not add points, and F must rise with tau.  The measured values are in DESIGN.md s8."""
    d = str(tmp_path / "dense")
    sc = synthetic.write_dense_folder(d, 64, 48, 4)
    before = native.cloud_launches()
    assert pipeline.run_dpe_pipeline(d, verbose=False, fusion=True) == 0
    assert native.cloud_launches() == before                              # the pipeline launched none
    recon = pipeline.read_point_cloud(os.path.join(d, "DPE", "DPE.ply"))
    gt = synthetic.gt_point_cloud(sc)
    foot = 5.0 / (1.2 * 64)
    taus = [foot, 2 * foot, 4 * foot, 8 * foot]
    e = pipeline.evaluate_clouds(recon, gt, taus, voxel=taus[3] / 2, gpu_index=0)
    assert native.cloud_launches() > before
    print("end to end, voxel = tau_max / 2: F =", e["fscore"], "precision", e["precision"], "recall", e["recall"],
          "points", e["n_recon_in"], "->", e["n_recon"], "gt", e["n_gt_in"], "->", e["n_gt"])
    assert e == pipeline.evaluate_clouds(recon, gt, taus, voxel=taus[3] / 2)
    assert e["n_recon"] <= e["n_recon_in"] == len(recon) and e["n_gt"] <= e["n_gt_in"] == len(gt)
    f = e["fscore"]
    assert all(f[k] <= f[k + 1] for k in range(3)) and f[3] > 0.0
