"""Voxel down-sampling on the host (host/cloud_voxel.cpp, host/ply_read.cpp, DPE_MVS.voxel, bin/dpe_voxel, the
--voxel / --crop options of the evaluation): dpe_host_cloud_voxel must give the bits of a numpy reference written
from the contract's text (tests/voxel_clouds.py) in xyz, rgb, first and count on clouds built to break it (points on
voxel faces, offsets of +-1000, one voxel of 20 000 points, non-finite points), with the properties a set-valued
result must have; the crop, the colour reader, the prepared evaluation and the command lines are held to their
contracts (include/dpe_host.h).  tests/test_cloud_voxel_gpu.py holds the device path to this host path."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from DPE_MVS import pipeline
from test_cloud_eval import MALFORMED, PKG, cloud_case, same_bits
from voxel_clouds import CASES, F, reference, voxel_case

NAMES = sorted(CASES)


def check_against(got, want, what):
    xyz, rgb, first, count = got
    wx, wc, wf, wn = want[:4]
    assert same_bits(first, wf), what
    assert same_bits(count, wn), what
    assert same_bits(xyz, wx), what
    assert (rgb is None and wc is None) or same_bits(rgb, wc), what


def rows(xyz, rgb, count):
    """The records as a sorted list of byte strings: their set, whatever the order."""
    parts = [np.ascontiguousarray(xyz).view(np.uint8).reshape(len(xyz), 12),
             np.ascontiguousarray(count).view(np.uint8).reshape(len(count), 4)]
    if rgb is not None:
        parts.append(np.ascontiguousarray(rgb).reshape(len(rgb), 3))
    return sorted(r.tobytes() for r in np.concatenate(parts, axis=1))


# ------------------------------------------------------------------------------ 1. the host path against the reference
@pytest.mark.parametrize("name", NAMES)
def test_host_matches_the_reference(name):
    P, v, Cc, plain, col = voxel_case(name)
    check_against(pipeline.voxel_down_sample(P, v), plain, name)
    check_against(pipeline.voxel_down_sample(P, v, Cc), col, name + " with colours")
    assert same_bits(plain[0], col[0])                                     # colours do not move a point


def test_the_cases_are_not_vacuous():
    """The conditions and figures of the clouds' table (the numpy reference)."""
    cnt = voxel_case("clustered_0.02")[3][3]
    print("clustered 0.02:", len(cnt), "voxels, share with >= 2 points", float((cnt >= 2).mean()), "largest", int(cnt.max()))
    assert len(cnt) == 47092 and (cnt >= 2).mean() >= 0.15 and cnt.max() >= 2000
    assert len(voxel_case("clustered_0.1")[3][3]) == 8078
    cnt = voxel_case("line_0.01")[3][3]
    assert len(cnt) == 3367 and cnt.max() >= 20000
    assert voxel_case("line_0.0025")[3][3].max() == 4125
    cnt = voxel_case("adversarial_R")[3][3]
    assert len(cnt) == 541 and cnt.min() >= 2
    cnt = voxel_case("adversarial_4R")[3][3]
    assert len(cnt) == 93 and cnt.max() == 204
    cnt = voxel_case("random")[3][3]
    assert len(cnt) == 64 and cnt.max() == 9 and 0.86 < (cnt >= 2).mean() < 0.88
    assert len(voxel_case("same")[3][3]) == 2 and voxel_case("same")[3][3].tolist() == [1000, 1]
    assert len(voxel_case("all_nan")[3][3]) == 0 and len(voxel_case("empty")[3][3]) == 0 and len(voxel_case("one")[3][3]) == 1
    cnt = voxel_case("lattice")[3][3]
    assert cnt.sum() == 3 * 23 * 5 and len(set(cnt.tolist())) > 2          # a face's three points do not stay together


@pytest.mark.parametrize("name", NAMES)
def test_properties(name):
    P, v, Cc, _, _ = voxel_case(name)
    xyz, rgb, first, count = pipeline.voxel_down_sample(P, v, Cc)
    fin = np.isfinite(P).all(axis=1)
    mean64 = voxel_case(name)[4][4]
    if fin.any():
        o = P[fin].astype(np.float64).min(axis=0)
        cells = np.floor((P[fin].astype(np.float64) - o) / np.float64(v)).astype(np.int64)
        uniq, inv = np.unique(cells, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        assert len(xyz) == len(uniq)                                       # one record per distinct cell
        lowest = np.full(len(uniq), len(P), np.int64)
        np.minimum.at(lowest, inv, np.nonzero(fin)[0])
        assert sorted(lowest.tolist()) == first.tolist()                   # each the lowest index of its cell
    else:
        assert len(xyz) == 0
    assert int(count.sum()) == int(fin.sum())
    assert (np.diff(first) > 0).all()
    if len(xyz):
        bound = np.float64(v) * 2.0 ** -31 + np.spacing(np.abs(mean64).astype(F)).astype(np.float64)
        err = np.abs(xyz.astype(np.float64) - mean64)
        print(name, "largest error over its bound", float((err / bound).max()))
        assert (err <= bound).all()
    # a shuffled input: the same set of records
    perm = np.random.default_rng(4).permutation(len(P))
    sx, sr, _, sc = pipeline.voxel_down_sample(P[perm], v, Cc[perm])
    assert rows(sx, sr, sc) == rows(xyz, rgb, count)
    # the cloud twice: the same points and colours, every count doubled
    dx, dr, df, dc = pipeline.voxel_down_sample(np.concatenate([P, P]), v, np.concatenate([Cc, Cc]))
    assert same_bits(dx, xyz) and same_bits(dr, rgb) and same_bits(df, first) and same_bits(dc, 2 * count)


# ------------------------------------------------------------------------------ 2. colour rounding
def test_colour_rounding():
    """Known sums: the mean rounded half up, (2 sum + count) / (2 count) in integers; the sums are 64 bits wide."""
    P = np.zeros((4, 3), F)
    for cols, want in [([0, 0, 0, 1], 0), ([0, 0, 1, 1], 1), ([0, 1, 1, 1], 1), ([1, 2, 2, 2], 2), ([254, 255, 255, 255], 255),
                       ([2, 3, 2, 3], 3), ([10, 11, 10, 12], 11)]:                # 0.25 0.5 0.75 1.75 254.75 2.5 10.75
        c = np.repeat(np.array(cols, np.uint8)[:, None], 3, axis=1)
        _, rgb, _, count = pipeline.voxel_down_sample(P, 1.0, c)
        assert count.tolist() == [4] and rgb.tolist() == [[want] * 3], cols
    _, rgb, _, _ = pipeline.voxel_down_sample(P[:2], 1.0, np.array([[0, 1, 2], [1, 2, 3]], np.uint8))
    assert rgb.tolist() == [[1, 2, 3]]                                      # x.5 goes up in every channel
    big = np.zeros((3000, 3), F)
    _, rgb, _, count = pipeline.voxel_down_sample(big, 1.0, np.full((3000, 3), 255, np.uint8))
    assert count.tolist() == [3000] and rgb.tolist() == [[255, 255, 255]]


# ------------------------------------------------------------------------------ 3. errors
def test_argument_errors():
    P = voxel_case("random")[0]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pipeline.PipelineError, match="cloud_voxel: bad argument"):
            pipeline.voxel_down_sample(P, bad)
    far = np.array([[-1e30, 0, 0], [1e30, 0, 0]], F)
    with pytest.raises(pipeline.PipelineError, match="voxel too small for the cloud's extent"):
        pipeline.voxel_down_sample(far, 1e-3)
    wide = np.array([[0, 0, 0], [2.0 ** 30, 0, 0]], F)                      # exactly 2^30 cells: refused; one less: fine
    with pytest.raises(pipeline.PipelineError, match="voxel too small for the cloud's extent"):
        pipeline.voxel_down_sample(wide, 1.0)
    assert len(pipeline.voxel_down_sample(np.array([[0, 0, 0], [2.0 ** 30 - 64, 0, 0]], F), 1.0)[0]) == 2


def test_cap_too_small_writes_nothing():
    P, v, _, plain, _ = voxel_case("random")
    k_want = len(plain[2])
    lib = pipeline.lib()
    xyz, first, count = np.full((k_want, 3), 7.5, F), np.full(k_want, -7, np.int32), np.full(k_want, -7, np.int32)
    k = C.c_size_t(12345)
    rc = lib.dpe_host_cloud_voxel(P.ctypes.data, len(P), None, float(v), xyz.ctypes.data, None, first.ctypes.data,
                                  count.ctypes.data, k_want - 1, C.byref(k))
    assert rc != 0 and k.value == k_want and "too small" in lib.dpe_pipeline_last_error().decode()
    assert (xyz == 7.5).all() and (first == -7).all() and (count == -7).all()
    rc = lib.dpe_host_cloud_voxel(P.ctypes.data, len(P), None, float(v), xyz.ctypes.data, None, first.ctypes.data,
                                  count.ctypes.data, k_want, C.byref(k))
    assert rc == 0 and k.value == k_want and same_bits(xyz, plain[0])


# ------------------------------------------------------------------------------ 4. crop
def test_crop():
    P = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [2, 2, 2], [0.5, 1.0000001, 0.5], [0.5, np.inf, 0.5],
                  [1, 0, 1], [-1e-9, 0.5, 0.5]], F)
    col = (np.arange(27).reshape(9, 3) * 7).astype(np.uint8)
    xyz, rgb, idx = pipeline.crop_cloud(P, [0, 0, 0], [1, 1, 1], col)
    assert idx.tolist() == [0, 1, 2, 7]                                     # both ends inclusive, NaN / inf dropped, order kept
    assert same_bits(xyz, P[idx]) and same_bits(rgb, col[idx])
    xyz, rgb, idx = pipeline.crop_cloud(P, [0, 0, 0], [1, 1, 1])
    assert rgb is None and idx.tolist() == [0, 1, 2, 7]
    assert pipeline.crop_cloud(P, [3, 3, 3], [4, 4, 4])[2].tolist() == []
    assert pipeline.crop_cloud(P, [-np.inf] * 3, [np.inf] * 3)[2].tolist() == [0, 1, 2, 4, 5, 7, 8]


# ------------------------------------------------------------------------------ 5. the colour reader
def test_colour_reader(tmp_path):
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.normal(0, 100, (500, 3)), rng.integers(0, 256, (500, 3))], axis=1).astype(F)
    path = str(tmp_path / "cloud.ply")
    pipeline.write_point_cloud(path, pts)
    xyz, bgr = pipeline.read_point_cloud_colors(path)                       # reads what the writer writes
    assert same_bits(xyz, pts[:, :3]) and same_bits(bgr, pts[:, 3:].astype(np.uint8))
    assert same_bits(pipeline.read_point_cloud(path), xyz)
    plain = tmp_path / "plain.ply"                                          # a file without colours says so
    plain.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                      b"property uchar red\nend_header\n1 2 3 9\n4 5 6 9\n")
    xyz, bgr = pipeline.read_point_cloud_colors(str(plain))
    assert bgr is None and xyz.tolist() == [[1, 2, 3], [4, 5, 6]]
    named = tmp_path / "named.ply"                                          # red / green / blue, ascii, in another order
    named.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 2\nproperty uchar red\nproperty float x\nproperty float y\n"
                      b"property uchar green\nproperty float z\nproperty uchar blue\nend_header\n10 1 2 20 3 30\n255 4 5 0 6 7\n")
    xyz, bgr = pipeline.read_point_cloud_colors(str(named))
    assert xyz.tolist() == [[1, 2, 3], [4, 5, 6]] and bgr.tolist() == [[30, 20, 10], [7, 0, 255]]
    data, message = MALFORMED["list"]                                       # refused as before
    bad = tmp_path / "list.ply"
    bad.write_bytes(data)
    with pytest.raises(pipeline.PipelineError, match=message):
        pipeline.read_point_cloud_colors(str(bad))
    data, message = MALFORMED["truncated_binary"]
    bad.write_bytes(data)
    with pytest.raises(pipeline.PipelineError, match=message):
        pipeline.read_point_cloud_colors(str(bad))


# ------------------------------------------------------------------------------ 6. the prepared evaluation
TODAY_KEYS = {"tau", "precision", "recall", "fscore", "radius", "mean_accuracy_truncated", "mean_completeness_truncated",
              "n_recon", "n_gt", "dropped_recon", "dropped_gt"}


def test_evaluate_without_the_new_arguments_is_unchanged():
    Q, T, _, _ = cloud_case("random")
    taus = [0.05, 0.1, 0.2]
    e = pipeline.evaluate_clouds(Q, T, taus, radius=0.25)
    assert set(e) == TODAY_KEYS
    # the numbers of the struct dpe_host_cloud_eval fills, key by key
    s = pipeline.DpeCloudEval()
    t = np.array(taus, F)
    assert pipeline.lib().dpe_host_cloud_eval(Q.ctypes.data, len(Q), T.ctypes.data, len(T), t.ctypes.data, 3, 0.25, -1, C.byref(s)) == 0
    assert e == dict(tau=[float(v) for v in s.tau[:3]], precision=list(s.precision[:3]), recall=list(s.recall[:3]),
                     fscore=list(s.fscore[:3]), radius=float(s.radius), mean_accuracy_truncated=s.mean_accuracy_truncated,
                     mean_completeness_truncated=s.mean_completeness_truncated, n_recon=257, n_gt=65, dropped_recon=0, dropped_gt=0)
    table = pipeline.format_cloud_eval(e)
    assert table.startswith("recon 257 points (0 dropped), gt 65 points (0 dropped), radius 0.25\n") and table.count("\n") == 7


def test_evaluate_with_voxel_and_crop():
    Q, T, _, _ = cloud_case("line")
    taus, v = [0.005, 0.01], 0.0025
    e = pipeline.evaluate_clouds(Q, T, taus, voxel=v)
    q, t = pipeline.voxel_down_sample(Q, v)[0], pipeline.voxel_down_sample(T, v)[0]
    base = pipeline.evaluate_clouds(q, t, taus)
    assert set(e) == TODAY_KEYS | {"voxel", "crop", "n_recon_in", "n_gt_in"}
    assert {k: e[k] for k in TODAY_KEYS} == base
    assert e["voxel"] == float(F(v)) and e["crop"] is None and e["n_recon_in"] == len(Q) and e["n_gt_in"] == len(T)
    assert e["n_recon"] == len(q) < len(Q) and e["n_gt"] == len(t) < len(T)
    lo, hi = [0.0, 0.0, 0.0], [1.0, 0.004, 0.004]
    e = pipeline.evaluate_clouds(Q, T, taus, voxel=v, crop=(lo, hi))           # cropped first, then down-sampled
    qc, tc = pipeline.crop_cloud(Q, lo, hi)[0], pipeline.crop_cloud(T, lo, hi)[0]
    assert 0 < len(qc) < len(Q) and 0 < len(tc) < len(T)
    base = pipeline.evaluate_clouds(pipeline.voxel_down_sample(qc, v)[0], pipeline.voxel_down_sample(tc, v)[0], taus)
    assert {k: e[k] for k in TODAY_KEYS} == base and e["crop"] == [[float(F(x)) for x in lo], [float(F(x)) for x in hi]]
    e = pipeline.evaluate_clouds(Q, T, taus, crop=(lo, hi))                    # a crop alone
    assert {k: e[k] for k in TODAY_KEYS} == pipeline.evaluate_clouds(qc, tc, taus) and e["voxel"] is None
    assert pipeline.format_cloud_eval(e).startswith("prepared: voxel 0, crop [0 0 0] to [1 ")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pipeline.PipelineError, match="voxel edge is not a finite positive"):
            pipeline.evaluate_clouds(Q, T, taus, voxel=bad)
    with pytest.raises(pipeline.PipelineError, match="crop box is empty"):
        pipeline.evaluate_clouds(Q, T, taus, crop=([1, 0, 0], [0, 1, 1]))


# ------------------------------------------------------------------------------ 7. the command lines
def write_ply(path, pts, col=None):
    pipeline.write_point_cloud(str(path), np.concatenate([pts, np.zeros_like(pts) if col is None else col.astype(F)], axis=1))


def prepared_files(tmp_path):
    """recon.ply, gt.ply, the options and evaluate_clouds' dict for them (shared with the device tests)."""
    Q, T, _, _ = cloud_case("line")
    write_ply(tmp_path / "recon.ply", Q)
    write_ply(tmp_path / "gt.ply", T)
    taus, v, lo, hi = [0.005, 0.01], 0.0025, [0.0, 0.0, 0.0], [50.0, 0.004, 0.004]
    want = pipeline.evaluate_clouds(Q, T, taus, voxel=v, crop=(lo, hi))
    return str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply"), taus, v, lo, hi, want


def test_evaluation_command_lines(tmp_path):
    recon, gt, taus, v, lo, hi, want = prepared_files(tmp_path)
    assert want["n_recon"] < want["n_recon_in"] and 0.0 < want["fscore"][0] <= want["fscore"][1]
    table = pipeline.format_cloud_eval(want)
    assert table.startswith("prepared: voxel 0.00249999994, crop [0 0 0] to [50 ")     # the float32 values, as the radius is printed
    box = [repr(x) for x in lo + hi]
    env = dict(os.environ, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, "-m", "DPE_MVS.evaluate", recon, gt, "--tau"] + [repr(t) for t in taus] +
                       ["--voxel", repr(v), "--crop"] + box + ["--cpu", "--json", str(tmp_path / "py.json")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == table
    got = json.load(open(tmp_path / "py.json"))
    assert got.pop("n_tau") == 2 and got == want
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_eval"), recon, gt] + [repr(t) for t in taus] +
                       ["--voxel", repr(v), "--crop"] + box + ["--cpu", "--json", str(tmp_path / "c.json")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == table
    got = json.load(open(tmp_path / "c.json"))
    assert got.pop("n_tau") == 2 and got == want


def test_thinning_command_lines(tmp_path):
    P, v, Cc, _, col = voxel_case("adversarial_R")
    write_ply(tmp_path / "in.ply", P, Cc)
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_voxel"), str(tmp_path / "in.ply"), str(tmp_path / "c.ply"), repr(float(v)),
                        "--cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "%d points -> %d points" % (len(P), len(col[0])) in r.stderr
    xyz, bgr = pipeline.read_point_cloud_colors(str(tmp_path / "c.ply"))      # reads back as the function's output
    assert same_bits(xyz, col[0]) and same_bits(bgr, col[1])
    r = subprocess.run([sys.executable, "-m", "DPE_MVS.voxel", str(tmp_path / "in.ply"), str(tmp_path / "py.ply"), repr(float(v)),
                        "--cpu"], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=PKG), timeout=120)
    assert r.returncode == 0, r.stderr
    assert "%d points -> %d points" % (len(P), len(col[0])) in r.stderr
    assert open(tmp_path / "py.ply", "rb").read() == open(tmp_path / "c.ply", "rb").read()
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_voxel"), str(tmp_path / "none.ply"), str(tmp_path / "x.ply"), "0.1", "--cpu"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot read" in r.stderr


# ------------------------------------------------------------------------------ 8. ASan + UBSan
@pytest.mark.timeout(600)
def test_host_voxel_and_colour_reader_under_asan_ubsan():
    """A stand-alone program (tests/sanitize/voxel_sanitize.cpp, linked with host/cloud_voxel.cpp and
    host/ply_read.cpp only) runs the host loop on an adversarial cloud, on 1 000 copies of one point and on non-finite
    points against its own serial check, the crop, and the colour reader on good and malformed files from memory;
    any report aborts it."""
    r = subprocess.run(["make", "-s", "sanitize-voxel"], cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(PKG, "bin", "voxel_sanitize")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "voxel sanitize ok" in r.stdout, r.stdout + r.stderr[-2000:]
