"""Cloud evaluation on the host (host/cloud_eval.cpp, host/ply_read.cpp, DPE_MVS.evaluate, bin/dpe_eval): the
grid path must give the bits of a brute-force float32 loop over the target in the contract's expression
order (include/dpe_mvs.h, dpe_cloud_nn), on clouds built to break a grid without a margin; the evaluation
must give exact fractions; the PLY reader must read what the writer writes and refuse malformed files with
its messages; the two command lines must print evaluate_clouds' numbers.  The clouds are shared with
tests/test_cloud_eval_gpu.py, which holds the device path to the host path."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from DPE_MVS import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dpe-mvs_amd")
F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def d2_rows(Q, t):
    """The contract's d2 of every query against one target point: float32, every operation rounded."""
    d = Q - t
    s = d[:, 0] * d[:, 0]
    s = s + d[:, 1] * d[:, 1]
    s = s + d[:, 2] * d[:, 2]
    return s


def brute(Q, T, R):
    """out[i] = min(R2, min_j d2(Q[i], T[j])): a float32 loop over the target."""
    Q, T = np.ascontiguousarray(Q, F).reshape(-1, 3), np.ascontiguousarray(T, F).reshape(-1, 3)
    R2 = F(R) * F(R)
    out = np.full(len(Q), R2, F)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in T:
            if not np.isfinite(t).all():
                continue
            s = d2_rows(Q, t)
            out = np.where(s < out, s, out)
    out[~np.isfinite(Q).all(axis=1)] = R2
    return out


# ------------------------------------------------------------------------------ the clouds (query, target, radius)
def random_cloud(seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((257, 3)).astype(F), rng.random((65, 3)).astype(F), 0.25


def random_cloud_wide(seed=0):
    """random_cloud with the queries drawn from the cube grown by R on every side: the input on which both
    kinds of value reach a quarter (see test_random_cloud)."""
    rng = np.random.default_rng(seed)
    T = rng.random((65, 3)).astype(F)
    return (rng.random((257, 3)) * 1.5 - 0.25).astype(F), T, 0.25


DIRECTIONS = [u for u in np.ndindex(3, 3, 3) if sum(1 for c in u if c != 1) in (1, 2, 3)]   # 6 axes, 12 face-, 8 diagonals


def adversarial_cloud():
    """About 5 000 points.  Targets around +1000 and -1000; queries at t + R u (1 - k 2^-24) for the 26
    directions and k in {0, 1, 2, 64}; queries at exact multiples of R, R (1 + 2^-23) and R (1 - 2^-23) from
    the target minimum."""
    R = F(0.0625) * F(1.1)
    rng = np.random.default_rng(5)
    T = np.concatenate([(rng.random((12, 3)) + 1000.0), (rng.random((12, 3)) - 1000.0),
                        (rng.random((12, 3)) * [1, 0, 1] + [1000.0, -1000.0, 0.0])]).astype(F)
    Q = []
    for t in T:
        for u in DIRECTIONS:
            u = np.array(u, np.float64) - 1.0
            u /= np.linalg.norm(u)
            for k in (0, 1, 2, 64):
                Q.append((t.astype(np.float64) + float(R) * u * (1.0 - k * 2.0 ** -24)).astype(F))
    lo = T.min(axis=0)
    for step in (R, R * F(1 + 2.0 ** -23), R * F(1 - 2.0 ** -23)):
        for i in range(-3, 40):
            Q.append(lo + F(i) * step)
            Q.append(lo + np.array([F(i) * step, 0, 0], F))
    # a target at the origin and queries (x, y, 0) whose float32 s is one ulp below R2, R2 itself and one ulp
    # above it: x among the neighbours of R, y^2 a few half-ulps of R2, found by trying
    T = np.concatenate([T, np.array([[0, 0, 0]], F)])
    R2 = R * R
    ulp = float(np.nextafter(R2, F(1))) - float(R2)
    for want in (np.nextafter(R2, F(0)), R2, np.nextafter(R2, F(1))):
        hits = [(x, y) for x in (R, np.nextafter(R, F(0)), np.nextafter(np.nextafter(R, F(0)), F(0)), np.nextafter(R, F(1)))
                for y in (F(np.sqrt(0.5 * k * ulp)) for k in range(12)) if x * x + y * y == want]
        assert hits, want
        x, y = hits[0]
        Q += [np.array([x, y, 0], F), np.array([0, -x, y], F)]
    return np.array(Q, F), T, float(R)


def line_cloud():
    """4 096 points spread over 10^4 R along one axis (more cells than buckets: 24 096 target points get 8 192
    buckets) and one cell holding 20 000 points (a long bucket); the queries are 400 of the line's points,
    moved a little, and 300 inside the crowded cell."""
    R = 0.01
    rng = np.random.default_rng(9)
    line = np.zeros((4096, 3))
    line[:, 0] = np.sort(rng.random(4096)) * 1e4 * R
    line[:, 1:] = rng.random((4096, 2)) * 0.5 * R
    crowd = np.array([50.25 * R, 0.1 * R, 0.1 * R]) + rng.random((20000, 3)) * 0.4 * R
    T = np.concatenate([line, crowd]).astype(F)
    Q = np.concatenate([line[::10][:400] + rng.normal(0, 0.4 * R, (400, 3)), crowd[:300] + rng.normal(0, 0.3 * R, (300, 3))])
    return Q.astype(F), T, R


def nonfinite_cloud():
    Q, T, R = random_cloud(3)
    Q, T = Q.copy(), T.copy()
    Q[0, 0], Q[5, 1], Q[9, 2], Q[11] = np.nan, np.inf, -np.inf, np.nan
    T[1, 2], T[2, 0], T[7, 1], T[8] = np.nan, -np.inf, np.inf, np.inf
    return Q, T, R


CLOUDS = {"random": random_cloud, "random_wide": random_cloud_wide, "adversarial": adversarial_cloud, "line": line_cloud,
          "nonfinite": nonfinite_cloud}
_cache = {}


def cloud_case(name):
    """(Q, T, R, brute(Q, T, R)), computed once and shared (read-only) by the tests of both files."""
    if name not in _cache:
        Q, T, R = CLOUDS[name]()
        want = brute(Q, T, R)
        for a in (Q, T, want):
            a.setflags(write=False)
        _cache[name] = (Q, T, R, want)
    return _cache[name]


# ------------------------------------------------------------------------------ 1. host path against brute force
@pytest.mark.parametrize("n,m", [(0, 5), (5, 0), (1, 1)])
def test_degenerate_sizes(n, m):
    rng = np.random.default_rng(1)
    Q, T = rng.random((n, 3)).astype(F), rng.random((m, 3)).astype(F)
    got = pipeline.cloud_nn(Q, T, 0.5)
    assert got.shape == (n,) and same_bits(got, brute(Q, T, 0.5))
    if m == 0:
        assert (got == F(0.25)).all()


def test_random_cloud():
    """257 x 65 uniform in the unit cube at R = 0.25: the host path has brute force's bits, and both truncated
    and untruncated values occur.  The share of truncated values on THIS input is about 6 % whatever the seed
    (a ball of radius 0.25 holds 65 * 4/3 pi 0.25^3 = 4.3 targets on average, so a query inside the cube is
    truncated with probability e^-4.3 = 1.4 %, more only near the faces): a quarter of each kind is out of
    its reach.  That share is asserted on random_cloud_wide, the same target and radius with the queries drawn
    from the cube grown by R on every side."""
    Q, T, R, want = cloud_case("random")
    got = pipeline.cloud_nn(Q, T, R)
    assert same_bits(got, want)
    assert (got == F(R) * F(R)).any() and (got < F(R) * F(R)).any()
    Q, T, R, want = cloud_case("random_wide")
    got = pipeline.cloud_nn(Q, T, R)
    assert same_bits(got, want)
    truncated = float((got == F(R) * F(R)).mean())
    print("random_wide: truncated share", truncated)
    assert truncated >= 0.25 and 1.0 - truncated >= 0.25


def test_adversarial_cloud():
    Q, T, R, want = cloud_case("adversarial")
    assert 4000 <= len(Q) + len(T) <= 6000
    # the set holds pairs whose float32 s is one ulp below R2, equal to R2 and one ulp above it
    R2 = F(R) * F(R)
    s = np.concatenate([d2_rows(Q, t) for t in T])
    for v in (np.nextafter(R2, F(0)), R2, np.nextafter(R2, F(1))):
        assert (s == v).any(), v
    got = pipeline.cloud_nn(Q, T, R)
    assert same_bits(got, want)
    assert (got == np.nextafter(R2, F(0))).any() and (got == R2).any()
    assert same_bits(pipeline.cloud_nn(T, Q, R), brute(T, Q, R))        # the other direction: the queries as the grid


def test_line_with_collisions_and_a_long_bucket():
    Q, T, R, want = cloud_case("line")
    got = pipeline.cloud_nn(Q, T, R)
    assert same_bits(got, want)
    assert (got < F(R) * F(R)).mean() > 0.5 and (got == F(R) * F(R)).any()


def test_nonfinite_points():
    Q, T, R, want = cloud_case("nonfinite")
    got = pipeline.cloud_nn(Q, T, R)
    assert same_bits(got, want)
    assert (got[[0, 5, 9, 11]] == F(R) * F(R)).all()
    only_bad = np.full((3, 3), np.nan, F)
    assert (pipeline.cloud_nn(Q, only_bad, R) == F(R) * F(R)).all()     # no finite target: all R2


def test_cloud_nn_argument_errors():
    Q, T, R, _ = cloud_case("random")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pipeline.PipelineError, match="bad argument"):
            pipeline.cloud_nn(Q, T, bad)
    far = np.array([[-1e30, 0, 0], [1e30, 0, 0]], F)
    with pytest.raises(pipeline.PipelineError, match="radius too small for the cloud's extent"):
        pipeline.cloud_nn(Q, far, 1e-3)
    assert same_bits(pipeline.cloud_nn(far, T, R), brute(far, T, R))    # far QUERIES are fine: clamped cells


# ------------------------------------------------------------------------------ 2. evaluate_clouds
def test_evaluate_identical_and_shifted():
    A = cloud_case("random")[0]
    tau = [0.0005, 0.001]         # far below the spacing of 257 random points: a shift of 10 tau meets no other point
    e = pipeline.evaluate_clouds(A, A, tau)
    assert e["precision"] == e["recall"] == e["fscore"] == [1.0, 1.0]
    assert e["mean_accuracy_truncated"] == 0.0 and e["mean_completeness_truncated"] == 0.0
    assert e["radius"] == float(F(0.001)) and e["n_recon"] == e["n_gt"] == 257 and e["dropped_recon"] == e["dropped_gt"] == 0
    e = pipeline.evaluate_clouds(A, A + F(10 * 0.001), tau)
    assert e["precision"] == e["recall"] == e["fscore"] == [0.0, 0.0]
    # every distance is truncated: the mean of n equal values sqrt((double)R2), summed in double (n roundings)
    want = float(np.sqrt(np.float64(F(0.001) * F(0.001))))
    assert e["mean_accuracy_truncated"] == pytest.approx(want, rel=257 * 2.0 ** -53)
    assert e["mean_completeness_truncated"] == pytest.approx(want, rel=257 * 2.0 ** -53)
    assert want == pytest.approx(0.001, rel=2.0 ** -23)      # = R up to the rounding of R * R


def test_evaluate_hand_computed_case():
    """Four reconstructed points at distances 0, 1, 2 and 10 from four ground-truth points, two of which no
    reconstructed point comes near; all on the integer lattice, so every distance is exact."""
    P = np.array([[0, 0, 0], [10, 0, 1], [20, 2, 0], [30, 10, 0]], F)
    G = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0]], F)
    e = pipeline.evaluate_clouds(P, G, [0.5, 1.5, 2.5], radius=4.0)
    assert e["precision"] == [0.25, 0.5, 0.75] and e["recall"] == [0.25, 0.5, 0.75]
    assert e["fscore"] == [0.25, 0.5, 0.75]
    assert e["mean_accuracy_truncated"] == (0 + 1 + 2 + 4) / 4 and e["mean_completeness_truncated"] == (0 + 1 + 2 + 4) / 4
    G2 = np.concatenate([G, [[100, 0, 0], [200, 0, 0], [300, 0, 0], [np.nan, 0, 0]]]).astype(F)
    e = pipeline.evaluate_clouds(P, G2, [1.5], radius=4.0)
    assert e["precision"] == [0.5] and e["recall"] == [0.25] and e["fscore"] == [2 * 0.5 * 0.25 / 0.75]
    assert e["dropped_gt"] == 1 and e["n_gt"] == 8 and e["mean_completeness_truncated"] == (0 + 1 + 2 + 4 * 5) / 8
    e = pipeline.evaluate_clouds(np.empty((0, 3), F), G, [1.0])                       # an empty reconstruction
    assert e["precision"] == e["recall"] == e["fscore"] == [0.0] and e["mean_accuracy_truncated"] == 0.0
    assert e["mean_completeness_truncated"] == 1.0


def test_evaluate_argument_errors():
    A = cloud_case("random")[0]
    with pytest.raises(pipeline.PipelineError, match="exceeds the radius"):
        pipeline.evaluate_clouds(A, A, [0.1, 0.3], radius=0.2)
    with pytest.raises(pipeline.PipelineError, match="1 to 16 thresholds"):
        pipeline.evaluate_clouds(A, A, [0.1] * 17)
    with pytest.raises(pipeline.PipelineError, match="1 to 16 thresholds"):
        pipeline.evaluate_clouds(A, A, [])
    assert len(pipeline.evaluate_clouds(A, A, [0.1] * 16)["fscore"]) == 16
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(pipeline.PipelineError, match="radius is not a finite positive"):
            pipeline.evaluate_clouds(A, A, [0.1], radius=bad)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(pipeline.PipelineError, match="threshold is not a finite positive"):
            pipeline.evaluate_clouds(A, A, [0.1, bad], radius=1.0)
    far = np.array([[-1e30, 0, 0], [1e30, 0, 0]], F)
    with pytest.raises(pipeline.PipelineError, match="radius too small for the cloud's extent"):
        pipeline.evaluate_clouds(A, far, [1e-3])


# ------------------------------------------------------------------------------ 3. the PLY reader
def ply(header_lines, body=b""):
    return ("\n".join(["ply"] + header_lines + ["end_header"]) + "\n").encode() + body


XYZ = ["property float x", "property float y", "property float z"]


def test_reader_round_trip_through_the_writer(tmp_path):
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.normal(0, 100, (1000, 3)), rng.integers(0, 256, (1000, 3))], axis=1).astype(F)
    pts[3, :3] = [np.nan, np.inf, -0.0]
    path = str(tmp_path / "cloud.ply")
    pipeline.write_point_cloud(path, pts)
    assert same_bits(pipeline.read_point_cloud(path), pts[:, :3])
    pipeline.write_point_cloud(path, np.empty((0, 6), F))
    assert pipeline.read_point_cloud(path).shape == (0, 3)


def test_reader_ascii_and_double_files(tmp_path):
    want = np.array([[1.5, -2.25, 3.0], [0.1, 1e-3, -7.0], [1000.5, 2.0, 0.125]], np.float64)
    a = tmp_path / "ascii.ply"
    a.write_bytes(ply(["format ascii 1.0", "comment by hand", "element vertex 3", "property uchar a"] + XYZ +
                      ["element face 1", "property list uchar int vertex_indices"],
                      b"5 1.5 -2.25 3\n6 0.1 1e-3 -7\r\n7 1000.5 2 0.125\n3 0 1 2\n"))
    assert same_bits(pipeline.read_point_cloud(str(a)), want.astype(F))
    d = tmp_path / "double.ply"
    body = b"".join(struct.pack("<Bhdidd", 9, -3, z, 11, x, y) for x, y, z in want)
    d.write_bytes(ply(["format binary_little_endian 1.0", "element camera 2", "property int id", "element vertex 3",
                       "property uchar red", "property short q", "property double z", "property int k", "property double x",
                       "property double y"], struct.pack("<ii", 7, 8) + body))
    assert same_bits(pipeline.read_point_cloud(str(d)), want.astype(F))      # 0.1 and 1e-3: doubles rounded to float


MALFORMED = {
    "list": (ply(["format ascii 1.0", "element vertex 1"] + XYZ + ["property list uchar int n"], b"0 0 0 0\n"), "list property"),
    "big_endian": (ply(["format binary_big_endian 1.0", "element vertex 1"] + XYZ, b"\0" * 12), "big-endian"),
    "truncated_binary": (ply(["format binary_little_endian 1.0", "element vertex 3"] + XYZ, b"\0" * 35), "truncated body"),
    "truncated_ascii": (ply(["format ascii 1.0", "element vertex 2"] + XYZ, b"0 0 0\n1 1\n"), "truncated body"),
    "count": (ply(["format ascii 1.0", "element vertex 2147483648"] + XYZ), "does not fit"),
    "huge_count": (ply(["format ascii 1.0", "element vertex 184467440737095516160"] + XYZ), "does not fit"),
    "negative_count": (ply(["format ascii 1.0", "element vertex -1"] + XYZ), "does not fit"),
    "missing_z": (ply(["format ascii 1.0", "element vertex 1"] + XYZ[:2], b"0 0\n"), "missing coordinate z"),
    "int_x": (ply(["format ascii 1.0", "element vertex 1", "property int x"] + XYZ[1:], b"0 0 0\n"), "neither float nor double"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_reader_refuses_malformed_files(tmp_path, case):
    data, message = MALFORMED[case]
    path = tmp_path / (case + ".ply")
    path.write_bytes(data)
    with pytest.raises(pipeline.PipelineError, match=message):
        pipeline.read_point_cloud(str(path))


def test_reader_missing_file(tmp_path):
    with pytest.raises(pipeline.PipelineError, match="cannot read"):
        pipeline.read_point_cloud(str(tmp_path / "none.ply"))


# ------------------------------------------------------------------------------ 4. the command lines
def write_xyz_ply(path, pts):
    pipeline.write_point_cloud(str(path), np.concatenate([pts, np.zeros_like(pts)], axis=1))


def eval_files(tmp_path):
    Q, T, _, _ = cloud_case("random")
    write_xyz_ply(tmp_path / "recon.ply", Q)
    write_xyz_ply(tmp_path / "gt.ply", T)
    taus = [0.05, 0.1, 0.2]
    return str(tmp_path / "recon.ply"), str(tmp_path / "gt.ply"), taus, pipeline.evaluate_clouds(Q, T, taus, radius=0.25)


def check_json(path, want):
    got = json.load(open(path))
    assert got.pop("n_tau") == len(want["tau"])
    assert got == want


def test_command_lines_print_evaluate_clouds_numbers(tmp_path):
    recon, gt, taus, want = eval_files(tmp_path)
    assert 0.0 < want["fscore"][0] < want["fscore"][2] < 1.0
    table = pipeline.format_cloud_eval(want)
    env = dict(os.environ, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, "-m", "DPE_MVS.evaluate", recon, gt, "--tau"] + [repr(t) for t in taus] +
                       ["--radius", "0.25", "--json", str(tmp_path / "py.json")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == table
    check_json(tmp_path / "py.json", want)
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_eval"), recon, gt] + [repr(t) for t in taus] +
                       ["--radius", "0.25", "--cpu", "--json", str(tmp_path / "c.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == table
    check_json(tmp_path / "c.json", want)
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_eval"), recon, str(tmp_path / "none.ply"), "0.1", "--cpu"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot read" in r.stderr


# ------------------------------------------------------------------------------ 5. ASan + UBSan
@pytest.mark.timeout(600)
def test_reader_and_host_grid_under_asan_ubsan():
    """A stand-alone program (tests/sanitize/cloud_sanitize.cpp, linked with host/ply_read.cpp and
    host/cloud_eval.cpp only) feeds the reader good files and each malformed case from memory-backed files and
    runs the host grid on a small adversarial cloud; any report aborts it."""
    r = subprocess.run(["make", "-s", "sanitize-cloud"], cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(PKG, "bin", "cloud_sanitize")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "cloud sanitize ok" in r.stdout, r.stdout + r.stderr[-2000:]
