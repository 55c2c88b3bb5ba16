"""Per-image point clouds (ExportDepthImagePointCloud, DPE.cpp:1691-1724) on the host: the serial loop
of dpe_host_depth_point_cloud against a numpy transcription, RescaleImageAndCamera, the pipeline's
point_<it>.ply files with a runner hook, and the two command lines' trailing argument.  Every
comparison is exact.  The device path is checked against these host functions in test_point_cloud_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from DPE_MVS import _abi, pipeline, synthetic
from test_pipeline import oracle_runner, _copy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dpe-mvs_amd")
F = np.float32
DMIN, DMAX = F(2.5), F(9.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cloud_camera(w, h):
    """A camera with a full rotation (every R entry non-zero) and an off-centre principal point."""
    ax, ay = 0.3, -0.2
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(0.1), -np.sin(0.1), 0], [np.sin(0.1), np.cos(0.1), 0], [0, 0, 1]])
    K = np.array([[1.3 * w, 0, 0.47 * w], [0, 1.1 * w, 0.55 * h], [0, 0, 1.0]])
    return synthetic.make_camera(K, Rx @ Ry @ Rz, np.array([0.4, -1.2, 2.6]), w, h, float(DMIN), float(DMAX))


def random_bgr(w, h, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


# the depths the range test must get right, with whether ExportDepthImagePointCloud keeps them in [DMIN, DMAX]
SPECIALS = [(DMIN, True), (DMAX, True), (np.nextafter(DMIN, F(-np.inf)), False), (np.nextafter(DMAX, F(np.inf)), False),
            (F(0), False), (F(-1), False), (F(np.nan), False), (F(np.inf), False), (F(-np.inf), False),
            (np.array([0xFFC00001], np.uint32).view(np.float32)[0], False),   # a negative NaN with a payload
            (np.array([0x7F800001], np.uint32).view(np.float32)[0], False)]   # a signalling NaN


def adversarial_depth(w, h, seed=1):
    """In-range depths with SPECIALS at known positions (a stride coprime to both sizes); the kept count."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(3.0, 8.0, (h, w)).astype(np.float32)
    flat = d.reshape(-1)
    pos = [(3 * k + 1) % flat.size for k in range(len(SPECIALS))]
    assert len(set(pos)) == len(pos)
    for q, (v, _) in zip(pos, SPECIALS):
        flat[q] = v
    return d, w * h - sum(1 for _, keep in SPECIALS if not keep)


def every_state_weak(w, h):
    """A weak map that holds every PixelState value and a byte that is none of them (from 4 pixels on;
    the first pixel is STRONG)."""
    k = ((np.arange(w * h) + 1) % 4).astype(np.uint8).reshape(h, w)
    k[k == 3] = 200
    assert k.flat[0] == _abi.STRONG and (w * h < 4 or {_abi.WEAK, _abi.STRONG, _abi.UNKNOWN, 200} <= set(np.unique(k).tolist()))
    return k


def numpy_cloud(depth, cam, bgr, dmin, dmax, mode=1, weak=None):
    """The double loop of DPE.cpp:1710-1721 with Get3DPointonWorld (DPE.cpp:1170-1194) in float32 scalars."""
    K = [F(v) for v in cam.K]
    R = [F(v) for v in cam.R]
    t = [F(v) for v in cam.t]
    h, w = depth.shape
    out = []
    with np.errstate(all="ignore"):
        Cx = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2])
        Cy = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2])
        Cz = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2])
        for i in range(w):
            for j in range(h):
                d = F(depth[j, i])
                if mode == 2 and weak[j, i] != _abi.STRONG:
                    d = F(0)
                if d < dmin or d > dmax or np.isnan(d):
                    continue
                px = d * (F(i) - K[2]) / K[0]
                py = d * (F(j) - K[5]) / K[4]
                pz = d
                tx = R[0] * px + R[3] * py + R[6] * pz
                ty = R[1] * px + R[4] * py + R[7] * pz
                tz = R[2] * px + R[5] * py + R[8] * pz
                out.append([tx + Cx, ty + Cy, tz + Cz, F(bgr[j, i, 0]), F(bgr[j, i, 1]), F(bgr[j, i, 2])])
    return np.array(out, np.float32).reshape(-1, 6)


# ------------------------------------------------------------------------------ 1. host function vs numpy
@pytest.mark.parametrize("w,h", [(7, 5), (5, 7)])
def test_host_loop_matches_numpy(w, h):
    depth, kept = adversarial_depth(w, h)
    cam, bgr = cloud_camera(w, h), random_bgr(w, h)
    got = pipeline.depth_point_cloud(depth, cam, bgr, DMIN, DMAX)
    want = numpy_cloud(depth, cam, bgr, DMIN, DMAX)
    assert len(want) == kept                                         # both ends kept, their neighbours and NaN / inf not
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    # column-major: the cloud begins with the points of the first COLUMN, top to bottom
    first_column = numpy_cloud(depth[:, :1], cam, bgr[:, :1], DMIN, DMAX)
    assert len(first_column) >= 2 and np.array_equal(bits(got[:len(first_column)]), bits(first_column))
    # mode 2: every PixelState value; a pixel that is not STRONG gets depth 0 and falls below depth_min
    weak = every_state_weak(w, h)
    got2 = pipeline.depth_point_cloud(depth, cam, bgr, DMIN, DMAX, mode="strong", weak=weak)
    want2 = numpy_cloud(depth, cam, bgr, DMIN, DMAX, 2, weak)
    assert 0 < len(want2) < kept and np.array_equal(bits(got2), bits(want2))
    # ... replaced, not dropped: with depth_min = 0 it is emitted at depth 0, as the reference's code would
    got0 = pipeline.depth_point_cloud(depth, cam, bgr, F(0), DMAX, mode=2, weak=weak)
    want0 = numpy_cloud(depth, cam, bgr, F(0), DMAX, 2, weak)
    assert len(want0) > len(want2) and len(want0) >= int((weak != _abi.STRONG).sum())
    assert np.array_equal(bits(got0), bits(want0))
    # cap: exact is enough, one short is an error
    assert len(pipeline.depth_point_cloud(depth, cam, bgr, DMIN, DMAX, cap=kept)) == kept
    with pytest.raises(pipeline.PipelineError):
        pipeline.depth_point_cloud(depth, cam, bgr, DMIN, DMAX, cap=kept - 1)
    with pytest.raises(pipeline.PipelineError):                      # mode 2 needs the states
        pipeline.depth_point_cloud(depth, cam, bgr, DMIN, DMAX, mode=2)


# ------------------------------------------------------------------------------ 2. RescaleImageAndCamera
@pytest.mark.parametrize("w,h", [(8, 6), (7, 5)])
def test_rescaled_camera_and_colour(w, h):
    sw, sh = 16, 12
    depth, _ = adversarial_depth(w, h)
    cam, bgr = cloud_camera(sw, sh), random_bgr(sw, sh)
    got = pipeline.depth_point_cloud(depth, cam, bgr, DMIN, DMAX)
    small = np.stack([pipeline.resize_u8(np.ascontiguousarray(bgr[:, :, k]), w, h) for k in range(3)], -1)
    scaled = pipeline.copy_camera(cam)
    sx, sy = F(w) / F(sw), F(h) / F(sh)                              # w / (float)src_w
    scaled.K[0], scaled.K[2] = F(cam.K[0]) * sx, F(cam.K[2]) * sx
    scaled.K[4], scaled.K[5] = F(cam.K[4]) * sy, F(cam.K[5]) * sy
    want = pipeline.depth_point_cloud(depth, scaled, small, DMIN, DMAX)
    assert len(want) > 0 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(want), bits(numpy_cloud(depth, scaled, small, DMIN, DMAX)))
    img, c = pipeline.rescale_image_and_camera(bgr, cam, w, h)
    assert np.array_equal(img, small) and bytes(c) == bytes(scaled)


def test_equal_sizes_leave_k_untouched():
    cam, bgr = cloud_camera(16, 12), random_bgr(16, 12)
    img, c = pipeline.rescale_image_and_camera(bgr, cam, 16, 12)
    assert np.array_equal(img, bgr) and bytes(c) == bytes(cam)


# ------------------------------------------------------------------------------ 3. pipeline, runner hook
@pytest.fixture(scope="module")
def dense4(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("points4"))
    synthetic.write_dense_folder(d, 64, 48, 4)
    return d


RUNNER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)


def recording_runner(folder, runner, states, ranges):
    """`runner` wrapped so that the test sees every pass: ranges[(id, it)] = the pass's depth range, and
    states[(id, it)] = the keep_intermediate maps a point-cloud pass left (they are overwritten by the next
    pass of the image, so they are read when that pass begins)."""
    base = RUNNER_FN(runner[0].value if isinstance(runner[0], C.c_void_p) else runner[0])

    def hook(user, inp_ptr, st):
        inp = C.cast(inp_ptr, C.POINTER(_abi.DpePassInput)).contents
        iid, it = int(inp.image_ids[0]), int(inp.pass_salt)
        ranges[(iid, it)] = (F(inp.params.depth_min), F(inp.params.depth_max))
        if it > 0 and it % 4 == 0:
            states[(iid, it - 1)] = read_state_maps(folder, iid)
        return base(user, inp_ptr, st)
    cb = RUNNER_FN(hook)
    return cb, (C.cast(cb, C.c_void_p).value, runner[1])


def read_state_maps(folder, iid):
    rf = os.path.join(folder, "DPE", f"{iid:08d}")
    return dict(depth=pipeline.read_bin_mat(os.path.join(rf, "depths.dmb")), weak=pipeline.read_bin_mat(os.path.join(rf, "weak.bin")))


def files_under(folder):
    out = {}
    for base, _, names in os.walk(os.path.join(folder, "DPE")):
        for f in names:
            p = os.path.join(base, f)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def check_ply(data):
    """The header's vertex count; the file is the header plus 15 bytes per vertex."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int(re.search(rb"element vertex (\d+)\n", data[:end]).group(1))
    assert len(data) == end + 15 * n
    return n


def expected_ply(tmp_path, folder, iid, state, rng, mode):
    cam = pipeline.read_camera(os.path.join(folder, "cams", f"{iid:08d}_cam.txt"))
    bgr = pipeline.read_bgr(os.path.join(folder, "images", f"{iid:08d}.jpg"))
    pts = pipeline.depth_point_cloud(state["depth"], cam, bgr, rng[0], rng[1], mode=mode, weak=state["weak"])
    p = str(tmp_path / "expected.ply")
    pipeline.write_point_cloud(p, pts)
    return open(p, "rb").read()


def check_point_cloud_run(tmp_path, folder, states, ranges, mode, n_images=4, n_iter=8):
    """point_<it>.ply exactly for (it + 1) % 4 == 0, each the PLY of that pass's state; returns the counts."""
    for i in range(n_images):
        states[(i, n_iter - 1)] = read_state_maps(folder, i)
    counts = {}
    for i in range(n_images):
        rf = os.path.join(folder, "DPE", f"{i:08d}")
        want_names = sorted(f"point_{it}.ply" for it in range(n_iter) if (it + 1) % 4 == 0)
        assert sorted(f for f in os.listdir(rf) if f.startswith("point_")) == want_names
        for it in range(3, n_iter, 4):
            data = open(os.path.join(rf, f"point_{it}.ply"), "rb").read()
            counts[(i, it)] = check_ply(data)
            st = states[(i, it)]
            assert data == expected_ply(tmp_path, folder, i, st, ranges[(i, it)], mode), (i, it)
            assert 0 < counts[(i, it)] <= st["depth"].size
    return counts


# one PatchMatch iteration per pass: the schedule, the sizes and the files are those of the full run
FAST = dict(verbose=False, keep_intermediate=True, max_iterations=1)


def test_pipeline_hook_writes_point_clouds(tmp_path, dense4):
    a = _copy(dense4, tmp_path, "on")
    b = _copy(dense4, tmp_path, "off")
    states, ranges = {}, {}
    keep, runner = recording_runner(a, oracle_runner(), states, ranges)
    assert pipeline.run_dpe_pipeline(a, runner=runner, normal=True, weak=True, point_cloud=1, **FAST) == 0
    assert len(ranges) == 4 * 8
    check_point_cloud_run(tmp_path, a, states, ranges, 1)
    assert states[(0, 3)]["depth"].shape == (24, 32) and states[(0, 7)]["depth"].shape == (48, 64)   # rescaled colour, then not
    # off: no file, and every other output as in the run with the option on
    assert pipeline.run_dpe_pipeline(b, runner=oracle_runner(), normal=True, weak=True, point_cloud="off", **FAST) == 0
    fa, fb = files_under(a), files_under(b)
    assert not [f for f in fb if "point_" in f]
    assert {f: v for f, v in fa.items() if "point_" not in f} == fb
    del keep


def test_pipeline_hook_strong_mode(tmp_path, dense4):
    """point_cloud = "strong": the points of the STRONG pixels only (the others get depth 0, below depth_min)."""
    c = _copy(dense4, tmp_path, "strong")
    states, ranges = {}, {}
    keep, runner = recording_runner(c, oracle_runner(), states, ranges)
    assert pipeline.run_dpe_pipeline(c, runner=runner, point_cloud="strong", **FAST) == 0
    counts = check_point_cloud_run(tmp_path, c, states, ranges, 2)
    for (i, it), n in counts.items():
        weak = states[(i, it)]["weak"]
        assert n == int((weak == _abi.STRONG).sum()) < weak.size, (i, it)
    del keep


def test_pipeline_refuses_a_bad_point_cloud(tmp_path, dense4):
    d = _copy(dense4, tmp_path, "bad")
    with pytest.raises(pipeline.PipelineError, match="point_cloud"):
        pipeline.run_dpe_pipeline(d, runner=oracle_runner(), verbose=False, point_cloud=3)
    with pytest.raises(ValueError, match="point_cloud"):
        pipeline.run_dpe_pipeline(d, runner=oracle_runner(), verbose=False, point_cloud="some")


# ------------------------------------------------------------------------------ 4. command lines
def test_command_lines_refuse_a_bad_point_cloud(tmp_path):
    exe = os.path.join(PKG, "bin", "dpe")
    r = subprocess.run([exe, str(tmp_path), "0", "0", "0", "0", "1", "0", "0", "0", "eth3d", "most"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "USAGE" in r.stderr and "point_cloud" in r.stderr
    r = subprocess.run([sys.executable, "-m", "DPE_MVS", str(tmp_path), "0", "0", "0", "0", "1", "0", "0", "0", "most"],
                       capture_output=True, text=True, timeout=120, cwd=PKG)
    assert r.returncode != 0 and "USAGE" in r.stderr and "point_cloud" in r.stderr
    from DPE_MVS.__main__ import main
    assert main(["DPE", str(tmp_path), "0", "0", "0", "0", "1", "0", "0", "0", "3"]) == 1
