"""Consistency maps (the option `consistency` = min_views): per reference pixel, the number of source
views for which RunFusion's view loop (DPE.cpp:1312-1343) reaches num_consistent++ with its masks[...]
tests and its blocks test removed, and the depth map filtered by that count.

The yardstick is the serial loop of host/consistency.cpp (dpe_host_consistency), which calls acosf
itself.  It is pinned three ways here: against the untouched oracle's oracle_fusion_candidates, against
the count histograms of a numpy float32 transcription, and against that transcription (np_consistency
below) on adversarial maps.  The device kernel is compared with it in tests/test_consistency_gpu.py.
Everything is bit-exact: no tolerance anywhere."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import oracle
from DPE_MVS import _abi, pipeline, synthetic
from test_fusion import _final_views, _free_port, oracle_runner, read_ply

F = np.float32
ANGLE_MAX = F(0.174533)


# ------------------------------------------------------------------------------ inputs
def gt_views(W, H, N):
    """[(depth, normal, DpeCamera)] of synthetic.make_scene's ground truth: depth with inf -> 0, world normals."""
    sc = synthetic.make_scene(W, H, N)
    return [(np.where(np.isfinite(v["depth"]), v["depth"], 0).astype(np.float32), v["normals"].astype(np.float32), cam)
            for v, cam in zip(sc["views"], sc["cams"])]


def simple_camera(w, h, f, cx, cy, R=(1, 0, 0, 0, 1, 0, 0, 0, 1), t=(0, 0, 0)):
    cam = _abi.DpeCamera()
    K = [f, 0, cx, 0, f, cy, 0, 0, 1]
    for i in range(9):
        cam.K[i], cam.R[i] = K[i], R[i]
    for i in range(3):
        cam.t[i] = t[i]
    cam.width, cam.height, cam.depth_min, cam.depth_max = w, h, 1.0, 10.0
    return cam


def adversarial_views(w, h):
    """A w x h reference view of the plane z = 4 and four source views, with in both depth maps NaN, +-inf,
    0, negative and denormal values, in both normal maps NaN, zero and length-2 normals (dot > 1 and < -1):
    view 1 the same camera shifted a little (most pixels agree), view 2 shifted by a third of a pixel with
    its normals tilted (the angle test decides), view 3 a camera turned round, behind the points, view 4 a
    camera with another image size."""
    bad =np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -4.0, 1e-40, 4.0], np.float32)

    def depth_map(ww, hh, shift):
        d = np.full(ww * hh, 4.0, np.float32)
        k = np.arange(ww * hh)
        sel = (k + shift) % 4 == 0
        d[sel] = bad[((k[sel] + shift) // 4) % len(bad)]
        return d.reshape(hh, ww)

    def normal_map(ww, hh, shift, tilt=0.0):
        n = np.zeros((ww * hh, 3), np.float32)
        n[:, 2] = -np.cos(tilt)
        n[:, 0] = np.sin(tilt)
        k = np.arange(ww * hh)
        n[(k + shift) % 7 == 0] = (np.nan, 0, -1)
        n[(k + shift) % 7 == 1] = (0, 0, 0)
        n[(k + shift) % 7 == 2] = (0, 0, -2)       # . (0, 0, -1) = 2 > 1: acosf NaN, GetAngle 0, passes
        n[(k + shift) % 7 == 3] = (0, 0, 2)        # . (0, 0, -1) = -2 < -1: the same
        return n.reshape(hh, ww, 3)

    f, cx, cy = 8.0, (w - 1) / 2, (h - 1) / 2
    views = [
        (depth_map(w, h, 0), normal_map(w, h, 0), simple_camera(w, h, f, cx, cy)),
        (depth_map(w, h, 1), normal_map(w, h, 2), simple_camera(w, h, f, cx, cy, t=(0.05, -0.03, 0.0))),
        (depth_map(w, h, 2), normal_map(w, h, 4, tilt=0.17), simple_camera(w, h, f, cx, cy, t=(0.17, 0.0, 0.01))),
        (depth_map(w, h, 3), normal_map(w, h, 5), simple_camera(w, h, f, cx, cy, R=(-1, 0, 0, 0, 1, 0, 0, 0, -1), t=(0, 0, 1.0))),
        (depth_map(w + 2, h - 1, 1), normal_map(w + 2, h - 1, 3), simple_camera(w + 2, h - 1, f * 1.25, cx + 1, cy - 0.5)),
    ]
    return views


# ------------------------------------------------------------------------------ the numpy float32 transcription
def _cam(cam):
    return (np.array(cam.K[:], np.float32), np.array(cam.R[:], np.float32), np.array(cam.t[:], np.float32))


def np_world(x, y, depth, cam):
    """Get3DPointonWorld (DPE.cpp:1170-1194), every operation rounded to float32, in its order."""
    K, R, t = _cam(cam)
    px = depth * (x.astype(np.float32) - K[2]) / K[0]
    py = depth * (y.astype(np.float32) - K[5]) / K[4]
    pz = depth
    tx = R[0] * px + R[3] * py + R[6] * pz
    ty = R[1] * px + R[4] * py + R[7] * pz
    tz = R[2] * px + R[5] * py + R[8] * pz
    cx = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2])
    cy = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2])
    cz = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2])
    return tx + cx, ty + cy, tz + cz


def np_project(X, cam):
    """ProjectCamera (DPE.cpp:1196-1206)."""
    K, R, t = _cam(cam)
    tx = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0]
    ty = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1]
    tz = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]
    depth = K[6] * tx + K[7] * ty + K[8] * tz
    return (K[0] * tx + K[1] * ty + K[2] * tz) / depth, (K[3] * tx + K[4] * ty + K[5] * tz) / depth, depth


def np_consistency(views, ref, src, min_views, D):
    """DPE.cpp:1303-1343 without the masks and the blocks, all pixels of view `ref` at once.  The angle test
    is `!(dot >= -1 && dot <= 1) || dot >= D`, which test 1 below shows equal to GetAngle(dot) < 0.174533f."""
    d_ref, n_ref, cam_r = views[ref]
    H, W = d_ref.shape
    r, c = np.mgrid[0:H, 0:W]
    count = np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        has_depth = d_ref > 0
        X = np_world(c, r, d_ref, cam_r)
        for s in src:
            d_s, n_s, cam_s = views[s]
            Hs, Ws = d_s.shape
            px, py, _ = np_project(X, cam_s)
            fx, fy = px + F(0.5), py + F(0.5)
            inside = has_depth & (fx > F(-1)) & (fx < F(Ws)) & (fy > F(-1)) & (fy < F(Hs))
            sc = np.where(inside, fx, F(0)).astype(np.int32)          # int(): towards zero
            sr = np.where(inside, fy, F(0)).astype(np.int32)
            sd = d_s[sr, sc]
            Y = np_world(sc, sr, sd, cam_s)
            tx, ty, pd2 = np_project(Y, cam_r)
            dx, dy = (c.astype(np.float32) - tx).astype(np.float64), (r.astype(np.float32) - ty).astype(np.float64)
            reproj = np.sqrt(dx * dx + dy * dy).astype(np.float32)      # pow(float, int): double, rounded once
            rel = np.abs(pd2 - d_ref) / d_ref
            sn = n_s[sr, sc]
            dot = n_ref[..., 0] * sn[..., 0] + n_ref[..., 1] * sn[..., 1] + n_ref[..., 2] * sn[..., 2]
            angle_ok = ~((dot >= F(-1)) & (dot <= F(1))) | (dot >= F(D))
            count += inside & (sd > 0) & (reproj < F(2)) & (rel < F(0.01)) & angle_ok
    filtered = np.where(count >= min_views, d_ref, F(0)).astype(np.float32)
    return count.astype(np.uint8), filtered


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------ 1. the threshold
def test_dot_threshold_is_the_angle_test():
    D = F(pipeline.consistency_dot_threshold())
    assert -1 < D < 1 and abs(D) > 1e-3
    bits = int(np.array([D]).view(np.int32)[0])
    near = (bits + np.arange(-4096, 4097)).astype(np.int32).view(np.float32)    # D > 0: the next float up is bits + 1
    assert D > 0 and np.all(np.diff(near) > 0) and near[4096] == D
    one, inf = F(1), F(np.inf)
    special = np.array([1, -1, 0.0, -0.0, inf, -inf, np.nan, np.nextafter(one, F(2)), np.nextafter(-one, F(-2))], np.float32)
    rnd = np.random.default_rng(20).uniform(-1.5, 1.5, 100000).astype(np.float32)
    for dots in (near, special, rnd):
        want = np.array([pipeline.consistency_angle_test(float(x)) for x in dots], bool)
        with np.errstate(invalid="ignore"):
            got = ~((dots >= F(-1)) & (dots <= F(1))) | (dots >= D)
        assert np.array_equal(got, want)
    assert pipeline.consistency_angle_test(float(D)) and not pipeline.consistency_angle_test(float(near[4095]))
    assert pipeline.consistency_angle_test(float("nan")) and pipeline.consistency_angle_test(2.0)   # GetAngle returns 0


# ------------------------------------------------------------------------------ 2. the host loop against the oracle
HISTOGRAMS = {(67, 45, 5): [89, 151, 539, 538, 1698], (64, 48, 4): [93, 323, 729, 1927]}


@pytest.mark.parametrize("shape", sorted(HISTOGRAMS))
def test_host_loop_matches_oracle_candidates(shape):
    W, H, N = shape
    views = gt_views(W, H, N)
    src = list(range(1, N))
    ns = len(src)
    count, kept2 = pipeline.consistency(views, 0, src, 2)
    idx, val = oracle.fusion_candidates(views, 0, src)
    idx, dot = idx.reshape(H * W, ns), val.reshape(H * W, ns, 3)[..., 2]
    angle = np.array([[pipeline.consistency_angle_test(float(x)) for x in row] for row in dot], bool)
    want = ((idx >= 0) & angle).sum(1).astype(np.uint8).reshape(H, W)
    assert same_bits(count, want)
    assert np.bincount(count.ravel(), minlength=ns + 1).tolist() == HISTOGRAMS[shape]   # every count value 0..ns occurs
    depth = views[0][0]
    for mv in (1, 2, ns + 1):
        c, f = pipeline.consistency(views, 0, src, mv)
        assert same_bits(c, count) and same_bits(f, np.where(count >= mv, depth, F(0)).astype(np.float32))
    assert 0 < np.count_nonzero(kept2) < W * H                       # (a condition on the input, not a tolerance)
    assert not pipeline.consistency(views, 0, src, ns + 1)[1].any()
    assert same_bits(count, np_consistency(views, 0, src, 2, pipeline.consistency_dot_threshold())[0])


def test_host_refuses_what_the_device_refuses():
    views = gt_views(16, 12, 3)
    for ref, src, mv in ((0, [1, 2], 0), (0, [1, 2], 256), (0, [1, 3], 1), (0, [-1], 1), (3, [1], 1), (0, [1, 0], 1),
                         (0, list(range(1, 3)) * 128, 1)):
        with pytest.raises(pipeline.PipelineError, match="consistency"):
            pipeline.consistency(views, ref, src, mv)
    c, f = pipeline.consistency(views, 0, [], 1)                      # ns = 0: nothing agrees
    assert c.shape == (12, 16) and not c.any() and not f.any()


# ------------------------------------------------------------------------------ 3. adversarial maps
@pytest.mark.parametrize("w,h", [(7, 5), (5, 7)])
def test_host_loop_matches_numpy_on_adversarial_maps(w, h):
    views = adversarial_views(w, h)
    D = pipeline.consistency_dot_threshold()
    seen = set()
    for src in ([1, 2, 3, 4], [4, 1], [3], [2]):
        for mv in (1, len(src)):
            count, filtered = pipeline.consistency(views, 0, src, mv)
            want_c, want_f = np_consistency(views, 0, src, mv, D)
            assert same_bits(count, want_c) and same_bits(filtered, want_f), (src, mv)
            seen |= set(count.ravel().tolist())
    assert {0, 1, 2}.issubset(seen)                                   # the maps are not all rejected
    # a source view as the reference: the other image size on the reference side
    count, filtered = pipeline.consistency(views, 4, [0, 1], 1)
    want_c, want_f = np_consistency(views, 4, [0, 1], 1, D)
    assert count.shape == (h - 1, w + 2) and same_bits(count, want_c) and same_bits(filtered, want_f) and count.any()


# ------------------------------------------------------------------------------ 4. the pipeline on the CPU
def _run(d, **kw):
    return pipeline.run_dpe_pipeline(d, runner=oracle_runner(), fusion_runner=oracle.fusion_runner(), verbose=False,
                                     keep_intermediate=True, **kw)


def consistency_files(d, n=4):
    return {(i, f): open(os.path.join(d, "DPE", f"{i:08d}", f), "rb").read()
            for i in range(n) for f in ("consistency.npy", "depth_filtered.npy")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The 64x48, 4-view folder run three times on the CPU (oracle passes, the host paths): with the option
    alone, with the option and fusion, and with fusion alone."""
    base = str(tmp_path_factory.mktemp("consistency"))
    out = {k: os.path.join(base, k) for k in ("only", "both", "fusion")}
    synthetic.write_dense_folder(out["only"], 64, 48, 4)
    for k in ("both", "fusion"):
        shutil.copytree(out["only"], out[k])
    assert _run(out["only"], consistency=1) == 0
    assert _run(out["both"], consistency=1, fusion=True) == 0
    assert _run(out["fusion"], fusion=True) == 0
    return out


def test_pipeline_writes_the_maps_of_its_final_states(runs):
    """Measured on this folder (CPU oracle passes, min_views = 1), count histograms [0, 1, 2, 3] per image:
    image 0 [2315, 423, 215, 119], image 1 [2419, 324, 200, 129], image 2 [2366, 365, 202, 139],
    image 3 [2535, 313, 124, 100] (the test prints them)."""
    for key in ("only", "both"):
        d = runs[key]
        views = _final_views(d, 4)
        vt = [(v["depth"], v["normal"], v["cam"]) for v in views]
        partial = 0
        for i, v in enumerate(views):
            rf = os.path.join(d, "DPE", f"{i:08d}")
            count, filtered = np.load(os.path.join(rf, "consistency.npy")), np.load(os.path.join(rf, "depth_filtered.npy"))
            assert count.dtype == np.uint8 and count.shape == (48, 64)
            assert filtered.dtype == np.dtype("<f4") and filtered.shape == (48, 64)
            want_c, want_f = pipeline.consistency(vt, i, v["src_ids"], 1)
            assert same_bits(count, want_c) and same_bits(filtered, want_f), i
            print(key, i, np.bincount(count.ravel(), minlength=4).tolist())
            partial += 0 < np.count_nonzero(count >= 1) < 64 * 48
        assert partial >= 1                                           # (a condition on the input)
    assert consistency_files(runs["only"]) == consistency_files(runs["both"])


def test_fusion_is_untouched_and_its_points_are_consistent(runs):
    a = open(os.path.join(runs["both"], "DPE", "DPE.ply"), "rb").read()
    assert a == open(os.path.join(runs["fusion"], "DPE", "DPE.ply"), "rb").read()
    xyz, _ = read_ply(os.path.join(runs["both"], "DPE", "DPE.ply"))
    assert len(xyz) > 100
    # every fused point is Get3DPointonWorld of a pixel some view agrees with: its count is >= 1
    consistent = set()
    for i, v in enumerate(_final_views(runs["both"], 4)):
        count = np.load(os.path.join(runs["both"], "DPE", f"{i:08d}", "consistency.npy"))
        r, c = np.nonzero(count >= 1)
        with np.errstate(all="ignore"):
            X = np.stack(np_world(c, r, v["depth"][r, c], v["cam"]), -1).astype(np.float32)
        consistent |= set(map(bytes, X.view(np.uint8).reshape(-1, 12)))
    assert all(bytes(p) in consistent for p in xyz.view(np.uint8).reshape(-1, 12))


def test_option_off_writes_neither_file(runs):
    names = [f for _, _, fs_ in os.walk(os.path.join(runs["fusion"], "DPE")) for f in fs_]
    assert "depth.npy" in names and "consistency.npy" not in names and "depth_filtered.npy" not in names


@pytest.mark.parametrize("value", [-1, 256])
def test_bad_option_fails_with_a_message(tmp_path, value):
    d = str(tmp_path / "bad")
    synthetic.write_dense_folder(d, 64, 48, 3)
    with pytest.raises(pipeline.PipelineError, match="consistency"):
        pipeline.run_dpe_pipeline(d, runner=oracle_runner(), verbose=False, consistency=value)


def test_cli_refuses_a_bad_consistency(tmp_path):
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dpe-mvs_amd", "bin", "dpe")
    for bad in ("256", "-1", "two"):
        r = subprocess.run([exe, str(tmp_path), "0", "0", "0", "0", "1", "0", "0", "0", "eth3d", "off", bad],
                           capture_output=True, text=True)
        assert r.returncode != 0 and "USAGE" in r.stderr and "consistency" in r.stderr


# ------------------------------------------------------------------------------ 5. ranks
def _rank_main(rank, world, port, folder):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        assert pipeline.run_dpe_pipeline(folder, runner=oracle_runner(), fusion_runner=oracle.fusion_runner(),
                                         verbose=False, dist=dist, consistency=2) == 0
    finally:
        dist.destroy_process_group()


def test_two_ranks_write_the_one_rank_files(tmp_path):
    import torch.multiprocessing as mp
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    synthetic.write_dense_folder(one, 64, 48, 4)
    shutil.copytree(one, two)
    assert pipeline.run_dpe_pipeline(one, runner=oracle_runner(), fusion_runner=oracle.fusion_runner(), schedule="jacobi",
                                     verbose=False, consistency=2) == 0
    mp.start_processes(_rank_main, args=(2, _free_port(), two), nprocs=2, join=True, start_method="spawn")
    a, b = consistency_files(one), consistency_files(two)
    assert len(a) == 8 and a == b
    assert any(np.load(os.path.join(one, "DPE", f"{i:08d}", "depth_filtered.npy")).any() for i in range(4))


# ------------------------------------------------------------------------------ 6. ABI
def test_options_struct_probes_the_default():
    o = pipeline.DpePipelineOptions()
    o.consistency = 77
    pipeline.lib().dpe_pipeline_default_options(C.byref(o))
    assert o.consistency == 0 and o.point_cloud == 0 and o.base_seed == 0x5EED
    assert pipeline.DpePipelineOptions.consistency.offset == pipeline.DpePipelineOptions.point_cloud.offset + 4
    t = (C.c_double * 9)(*([-1.0] * 9))
    assert pipeline.lib().dpe_pipeline_last_timings(t, 8) == 8 and t[8] == -1.0      # callers that pass 8 see 8
    assert pipeline.lib().dpe_pipeline_last_timings(t, 16) == 9 and t[8] >= 0.0      # [8]: the consistency maps
