"""Rigid registration on the host (host/cloud_register.cpp, host/cloud_eval.cpp, DPE_MVS.register, bin/dpe_register,
the --register options of the evaluation): the nearest neighbour with index and one ICP step must give the bits of
numpy references written from the contract's text (include/dpe_mvs.h: lexicographic (d2, j); float64 terms summed by
the pairwise tree in index order), the solve must agree with numpy's SVD Kabsch, the loop must recover a known motion
to the float rounding of its inputs, the refusals must write nothing, and the evaluation and the command lines must
print what the functions return.  tests/test_cloud_register_gpu.py holds the device path to this host path."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from DPE_MVS import pipeline
from test_cloud_eval import CLOUDS, PKG, cloud_case, d2_rows, same_bits
from test_cloud_voxel import prepared_files, write_ply

F = np.float32
EPS = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------ the references (numpy, from the contract)
def brute_index(Q, T, R):
    """(d2, idx): the j that minimises (d2(Q[i], T[j]), j) lexicographically over the finite T[j] with d2 < R2, -1
    without one.  Targets are visited in ascending j and only a strictly smaller d2 replaces the pair."""
    Q, T = np.ascontiguousarray(Q, F).reshape(-1, 3), np.ascontiguousarray(T, F).reshape(-1, 3)
    best = np.full(len(Q), F(R) * F(R), F)
    idx = np.full(len(Q), -1, np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j, t in enumerate(T):
            if not np.isfinite(t).all():
                continue
            s = d2_rows(Q, t)
            take = s < best
            best = np.where(take, s, best)
            idx = np.where(take, np.int32(j), idx)
    bad = ~np.isfinite(Q).all(axis=1)
    best[bad], idx[bad] = F(R) * F(R), -1
    return best, idx


def apply_ref(T, P):
    """x' = (float)(((T0 x + T1 y) + T2 z) + T3) per row, float64 operations in this order; NaN for a non-finite point."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    p = np.asarray(P, F).astype(np.float64)
    out = np.empty((len(p), 3), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            s = T[r, 0] * p[:, 0]
            s = s + T[r, 1] * p[:, 1]
            s = s + T[r, 2] * p[:, 2]
            s = s + T[r, 3]
            out[:, r] = s.astype(F)
    out[~np.isfinite(P).all(axis=1)] = np.nan
    return out


def minima(P):
    fin = np.isfinite(P).all(axis=1)
    return P[fin].astype(np.float64).min(axis=0) if fin.any() else np.zeros(3)


def pairwise(terms):
    """The contract's tree over the rows: s = s[0::2] + s[1::2] after padding an odd length with +0.0."""
    s = np.array(terms, np.float64)
    while len(s) > 1:
        if len(s) % 2:
            s = np.concatenate([s, np.zeros((1, s.shape[1]))])
        s = s[0::2] + s[1::2]
    return s[0]


def step_ref(P, G, d2, idx):
    """(matched, 16 sums) of one step from the match (d2, idx) of the transformed source."""
    P, G = np.asarray(P, F), np.asarray(G, F)
    terms = np.zeros((len(P), 16), np.float64)
    m = idx >= 0
    a = P[m].astype(np.float64) - minima(P)
    b = G[idx[m]].astype(np.float64) - minima(G)
    terms[m, 0] = d2[m].astype(np.float64)
    terms[m, 1:4], terms[m, 4:7] = a, b
    for r in range(3):
        for c in range(3):
            terms[m, 7 + 3 * r + c] = a[:, r] * b[:, c]
    return int(m.sum()), pairwise(terms)


def sums_vector(s):
    return np.array([s["d2"]] + s["a"] + s["b"] + s["ab"], np.float64)


def rotation(axis, degrees):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def kabsch(P, G):
    """The float64 SVD solution [R | t] of min sum |R p + t - g|^2 over proper rotations."""
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    pm, gm = P.mean(axis=0), G.mean(axis=0)
    U, S, Vt = np.linalg.svd((P - pm).T @ (G - gm))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return np.concatenate([R, (gm - R @ pm)[:, None]], axis=1), S


R0, T0 = rotation([1, 2, 3], 4.0), np.array([0.03, -0.02, 0.01])
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


# ------------------------------------------------------------------------------ the clouds of the index checks
def tie_same_point():
    """The same target point at indices 7 and 3, nearest to every query: index 3 wins."""
    rng = np.random.default_rng(11)
    T = (rng.random((12, 3)) + 2.0).astype(F)
    T[7] = T[3] = [0.5, 0.5, 0.5]
    return (rng.random((70, 3)) * 0.2 + 0.4).astype(F), T, 1.0


def tie_mirror():
    """A query at the origin between targets at (+-1, 0, 0): equal d2, the lower index wins, whichever side it is on."""
    return np.zeros((1, 3), F), np.array([[5, 5, 5], [1, 0, 0], [-1, 0, 0], [1, 0, 0]], F), 1.5


def empty_target():
    return CLOUDS["random"]()[0], np.empty((0, 3), F), 0.25


INDEX_CLOUDS = dict(CLOUDS, tie_same_point=tie_same_point, tie_mirror=tie_mirror, empty_target=empty_target)
_index_cache = {}


def index_case(name):
    """(Q, T, R, d2, idx) with the numpy reference, computed once and shared (read-only) with the device tests."""
    if name not in _index_cache:
        Q, T, R = cloud_case(name)[:3] if name in CLOUDS else INDEX_CLOUDS[name]()
        d2, idx = brute_index(Q, T, R)
        for a in (d2, idx):
            a.setflags(write=False)
        _index_cache[name] = (Q, T, R, d2, idx)
    return _index_cache[name]


# ------------------------------------------------------------------------------ 1. index against numpy
@pytest.mark.parametrize("name", sorted(INDEX_CLOUDS))
def test_index_against_numpy(name):
    Q, T, R, want_d2, want_idx = index_case(name)
    d2, idx = pipeline.cloud_nn_index(Q, T, R)
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx)
    assert same_bits(d2, want_d2) and same_bits(d2, pipeline.cloud_nn(Q, T, R))
    assert ((idx >= 0) == (d2 < F(R) * F(R))).all()
    if name == "tie_same_point":
        assert (idx == 3).all()
    if name == "tie_mirror":
        assert idx.tolist() == [1]
    if name == "empty_target":
        assert (idx == -1).all()
    if name == "nonfinite":
        assert (idx[[0, 5, 9, 11]] == -1).all() and not np.isin(idx, [1, 2, 7, 8]).any()
    if name in ("adversarial", "line", "random_wide"):
        assert (idx >= 0).any() and (idx == -1).any()


# ------------------------------------------------------------------------------ 2. step against numpy
STEP_SIZES = [1, 2, 3, 255, 256, 257, 4097, 65537]
STEP_R = 0.05
T_ROT = np.concatenate([rotation([3, -1, 2], 1.5), np.array([[0.004], [-0.003], [0.002]])], axis=1)
_step_cache = {}


def step_clouds():
    """G: 2 000 points of the unit cube.  `third`: 65 537 sources, each a target point moved by up to 0.4 R per axis, every
    third one lifted by 1.2 in z, out of the cube and beyond R of every target.  `far`: sources more than 1 away from
    every target.
    `nonfinite`: `third` with NaN and inf sprinkled in.  Prefixes of these serve every size."""
    if "clouds" not in _step_cache:
        rng = np.random.default_rng(77)
        G = rng.random((2000, 3)).astype(F)
        n = max(STEP_SIZES)
        P = G[rng.integers(0, len(G), n)].astype(np.float64) + (rng.random((n, 3)) - 0.5) * 0.8 * STEP_R
        P[np.arange(n) % 3 == 1, 2] += 1.2
        third = P.astype(F)
        far = (rng.random((n, 3)) + [3.0, 0.0, 0.0]).astype(F)
        bad = third.copy()
        bad[::7, 0], bad[3::11, 1], bad[5::13] = np.nan, np.inf, -np.inf
        for a in (G, third, far, bad):
            a.setflags(write=False)
        _step_cache["clouds"] = dict(G=G, third=third, far=far, nonfinite=bad)
    return _step_cache["clouds"]


def step_match(kind, T):
    """brute_index of all 65 537 transformed sources of `kind`, once per (kind, T): a prefix of the sources has the
    prefix of the match."""
    key = (kind, np.asarray(T).tobytes())
    if key not in _step_cache:
        c = step_clouds()
        _step_cache[key] = brute_index(apply_ref(T, c[kind]), c["G"], STEP_R)
    return _step_cache[key]


@pytest.mark.parametrize("name,T", [("identity", IDENTITY), ("rotated", T_ROT)])
def test_step_against_numpy(name, T):
    c = step_clouds()
    d2, idx = step_match("third", T)
    share = float((idx < 0).mean())
    print(name, "unmatched share", share)
    assert 0.33 < share < (0.34 if name == "identity" else 0.6)            # a third lies beyond R (more once T moves the rest)
    for n in STEP_SIZES:
        P = c["third"][:n]
        assert same_bits(pipeline.transform_cloud(T, P), apply_ref(T, P))
        want_n, want = step_ref(P, c["G"], d2[:n], idx[:n])
        got = pipeline.cloud_icp_step(P, c["G"], STEP_R, T)
        assert got["matched"] == want_n, n
        assert same_bits(sums_vector(got), want), (n, sums_vector(got) - want)
    assert want_n > 40000 and (want > 0.0).all()


def test_step_all_unmatched_is_plus_zero():
    c = step_clouds()
    d2, idx = brute_index(c["far"][:4097], c["G"], STEP_R)
    assert (idx == -1).all()
    for n in STEP_SIZES:
        got = pipeline.cloud_icp_step(c["far"][:n], c["G"], STEP_R, IDENTITY)
        assert got["matched"] == 0
        assert same_bits(sums_vector(got), np.zeros(16)), n                # +0.0, not -0.0
    got = pipeline.cloud_icp_step(c["third"][:300], np.empty((0, 3), F), STEP_R, IDENTITY)    # an empty target
    assert got["matched"] == 0 and same_bits(sums_vector(got), np.zeros(16))


def test_step_nonfinite_sources_do_not_match():
    c = step_clouds()
    n = 4097
    P = c["nonfinite"][:n]
    d2, idx = brute_index(apply_ref(T_ROT, P), c["G"], STEP_R)
    assert (idx[~np.isfinite(P).all(axis=1)] == -1).all()
    want_n, want = step_ref(P, c["G"], d2, idx)
    got = pipeline.cloud_icp_step(P, c["G"], STEP_R, T_ROT)
    assert got["matched"] == want_n and same_bits(sums_vector(got), want)
    huge = np.concatenate([IDENTITY[:, :3] * 1e38, np.zeros((3, 1))], axis=1)         # images overflow to inf: no match
    got = pipeline.cloud_icp_step(c["third"][:257] + F(10), c["G"], STEP_R, huge)
    assert got["matched"] == 0 and same_bits(sums_vector(got), np.zeros(16))


# ------------------------------------------------------------------------------ 3. solve against numpy SVD
def solve_clouds():
    """Four clouds of unit extent, 500 points each with axes scaled (1, 0.7, 0.4) so that the singular values of H lie
    within a factor of 10 and apart; a motion, noise of 0.01; the last one mirrored in z, so that the SVD solution needs
    its sign fix."""
    out = []
    for k, (axis, deg, t, off) in enumerate([([1, 0, 0], 10, [0.1, 0.2, -0.3], 0.0), ([1, 2, 3], 75, [5, -3, 2], 0.0),
                                              ([-2, 1, 0.5], 170, [0, 0, 0], 1000.0), ([0, 1, 1], 33, [-1, 0.5, 0.25], 0.0)]):
        rng = np.random.default_rng(100 + k)
        P = rng.random((500, 3)) * [1.0, 0.7, 0.4] + off
        G = P @ rotation(axis, deg).T + t + rng.normal(0, 0.01, P.shape)
        if k == 3:
            G[:, 2] = -G[:, 2]
        out.append((P, G))
    return out


def test_solve_against_svd():
    """dpe_host_cloud_solve from float64 sums of all pairs against numpy's SVD Kabsch on the same pairs.  Measured here:
    largest |T - T_svd| over the four clouds 2.2e-12 (one cloud sits at an offset of 1000, which t multiplies into the
    rotation's last bits), largest |R^T R - I| 2.2e-16, largest |det R - 1| 4.4e-16; the bound of 1e-9 on T is loose on purpose (a failure is a wrong solve, not an imprecise one),
    the bounds on R are 64 double epsilons."""
    worst_t = worst_o = worst_d = 0.0
    for k, (P, G) in enumerate(solve_clouds()):
        o_s, o_t = P.min(axis=0), G.min(axis=0)
        a, b = P - o_s, G - o_t
        sums = dict(matched=len(P), d2=0.0, a=a.sum(axis=0).tolist(), b=b.sum(axis=0).tolist(), ab=(a.T @ b).reshape(-1).tolist())
        T = pipeline.cloud_solve(sums, o_s, o_t)
        want, S = kabsch(P, G)
        U, _, Vt = np.linalg.svd((P - P.mean(axis=0)).T @ (G - G.mean(axis=0)))
        print("cloud", k, "singular values", S, "det(V U^T)", np.linalg.det(Vt.T @ U.T))
        assert (np.linalg.det(Vt.T @ U.T) < 0) == (k == 3)                  # the mirrored cloud needs the sign fix
        assert S[0] / S[2] < 10.0
        R = T[:, :3]
        worst_o = max(worst_o, float(np.abs(R.T @ R - np.eye(3)).max()))
        worst_d = max(worst_d, abs(float(np.linalg.det(R)) - 1.0))
        worst_t = max(worst_t, float(np.abs(T - want).max()))
        assert np.abs(R.T @ R - np.eye(3)).max() < 64 * EPS and abs(np.linalg.det(R) - 1.0) < 64 * EPS
        assert np.abs(T - want).max() < 1e-9, k
    print("largest |T - T_svd|", worst_t, "|R^T R - I|", worst_o, "|det R - 1|", worst_d)


# ------------------------------------------------------------------------------ 4. the loop recovers a known motion
_motion = {}


def motion_case():
    """(P, G, sel): G 4 000 points of a wavy sheet over the unit square, P = G[sel] (1 500 of them) moved by the inverse of
    (R0, t0), as float32.  Shared with the device tests and tools/cloud_eval_prof.py's --register."""
    if not _motion:
        rng = np.random.default_rng(20261020)
        x, y = rng.random(4000), rng.random(4000)
        G = np.stack([x, y, 0.1 * np.sin(3 * x) * np.cos(2 * y) + 0.05 * np.sin(11 * x + 1) * np.sin(7 * y)], axis=1).astype(F)
        sel = rng.permutation(4000)[:1500]
        P = ((G[sel].astype(np.float64) - T0) @ R0).astype(F)               # R0^T (g - t0)
        for a in (P, G, sel):
            a.setflags(write=False)
        _motion.update(P=P, G=G, sel=sel)
    return _motion["P"], _motion["G"], _motion["sel"]


def test_loop_recovers_a_known_motion():
    P, G, sel = motion_case()
    want, _ = kabsch(P, G[sel])
    print("Kabsch on the true pairs against (R0, t0):", np.abs(want - np.concatenate([R0, T0[:, None]], axis=1)).max())
    assert np.abs(want[:, 3] - T0).max() < 1e-9
    one = pipeline.register_clouds(P, G, 0.15, max_iters=50)
    st = one["stages"]
    print("one stage:", st)
    assert len(st) == 1 and st[0]["converged"] == 2 and st[0]["matched"] == 1500 and st[0]["iters"] <= 50
    assert st[0]["radius"] == float(F(0.15)) and st[0]["rms"] < 1e-7
    T = np.array(one["T"])
    assert np.abs(T - want).max() < 1e-9
    assert np.array_equal(pipeline.cloud_nn_index(pipeline.transform_cloud(T, P), G, 0.15)[1], sel)     # the true matches
    two = pipeline.register_clouds(P, G, [0.3, 0.05], max_iters=50)
    print("two stages:", two["stages"])
    assert [s["converged"] for s in two["stages"]] == [2, 2] and [s["matched"] for s in two["stages"]] == [1500, 1500]
    assert np.abs(np.array(two["T"]) - want).max() < 1e-9
    # 300 more sources above the sheet, more than 1 from every target and inside the source's bounds in x and y: they
    # never match, leave the minima alone and sit at the end of the index order, where +0.0 terms change no node
    rng = np.random.default_rng(5)
    extra = np.concatenate([rng.random((300, 2)) * 0.6 + 0.2, rng.random((300, 1)) + 2.0], axis=1).astype(F)
    more = pipeline.register_clouds(np.concatenate([P, extra]), G, 0.15, max_iters=50)
    assert more["stages"] == st and same_bits(np.array(more["T"]), T)
    assert pipeline.register_clouds(P, G, 0.15, init=one["T"])["stages"][0]["iters"] == 2                # a fixed point stays one


# ------------------------------------------------------------------------------ 5. error cases
def test_error_cases_write_nothing():
    P, G, _ = motion_case()
    lib = pipeline.lib()

    def refused(message, src=P, n=len(P), tgt=G, m=len(G), n_radii=None, **kw):
        o = pipeline._reg_options(kw.pop("radii", [0.15]), **kw)
        if n_radii is not None:
            o.n_radii = n_radii
        out = pipeline.DpeCloudReg()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        rc = lib.dpe_host_cloud_register(None if src is None else src.ctypes.data, n, None if tgt is None else tgt.ctypes.data, m,
                                         C.byref(o), -1, C.byref(out))
        assert rc != 0 and message in lib.dpe_pipeline_last_error().decode(), lib.dpe_pipeline_last_error()
        assert bytes(out) == b"\x5A" * C.sizeof(out)                       # nothing written
    refused("fewer than 3 matches within the radius", src=(P + F(50)))
    refused("fewer than 3 matches within the radius", src=P[:2], n=2, radii=[5.0])
    for bad in (0.0, float("nan"), float("inf"), -1.0):
        refused("radius is not a finite positive", radii=[0.3, bad])
    for k in (0, 5):
        refused("1 to 4 radii", n_radii=k)
    refused("1 to 1000 iterations", max_iters=0)
    refused("1 to 1000 iterations", max_iters=1001)
    refused("tolerance", tol=-1.0)
    refused("bad argument", src=None)
    refused("bad argument", tgt=None)
    refused("bad argument", n=2 ** 31)
    refused("bad argument", m=2 ** 31)
    refused("radius too small for the cloud's extent", tgt=np.array([[-1e30, 0, 0], [1e30, 0, 0]], F), m=2, radii=[1e-3])
    s = pipeline.DpeIcpSums()
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    for args in ((None, len(P), G.ctypes.data, len(G), 0.15), (P.ctypes.data, 2 ** 31, G.ctypes.data, len(G), 0.15),
                 (P.ctypes.data, len(P), G.ctypes.data, len(G), 0.0), (P.ctypes.data, len(P), G.ctypes.data, len(G), float("nan"))):
        assert lib.dpe_host_cloud_icp_step(*args, IDENTITY.ctypes.data, C.byref(s)) != 0
        assert "cloud_icp_step: bad argument" in lib.dpe_pipeline_last_error().decode() and bytes(s) == b"\x5A" * C.sizeof(s)
    with pytest.raises(pipeline.PipelineError, match="cloud_nn_index: bad argument"):
        pipeline.cloud_nn_index(P, G, 0.0)
    with pytest.raises(pipeline.PipelineError, match="fewer than 3 matches"):
        pipeline.evaluate_clouds(P + F(50), G, [0.01], register=0.15)
    assert pipeline.register_clouds(P, G, 0.15)["stages"][0]["converged"] == 2                           # still usable


# ------------------------------------------------------------------------------ 6. evaluation and command lines
REGISTER = dict(radii=[8.0, 0.5, 0.02], max_iters=100)


def registered_files(tmp_path):
    """test_cloud_voxel.prepared_files with the reconstruction moved by (R0, t0)^-1, and evaluate_clouds' dict with the
    registration (shared with the device tests).  The line cloud is a poor registration problem (the crop keeps half of
    the ground truth's line), so nothing is asked of T here beyond what the functions return for it."""
    recon, gt, taus, v, lo, hi, _ = prepared_files(tmp_path)
    Q, T, _, _ = cloud_case("line")
    moved = ((Q.astype(np.float64) - T0) @ R0).astype(F)
    write_ply(tmp_path / "recon.ply", moved)
    want = pipeline.evaluate_clouds(moved, T, taus, voxel=v, crop=(lo, hi), register=REGISTER)
    return recon, gt, taus, v, lo, hi, moved, T, want


def register_flags():
    return ["--register"] + [repr(r) for r in REGISTER["radii"]] + ["--register-iters", str(REGISTER["max_iters"])]


def test_evaluation_with_registration(tmp_path):
    recon, gt, taus, v, lo, hi, moved, T, want = registered_files(tmp_path)
    reg = want["registration"]
    assert set(reg) == {"T", "stages"} and len(reg["T"]) == 3 and all(len(r) == 4 for r in reg["T"])
    assert [set(s) for s in reg["stages"]] == [{"radius", "iters", "matched", "rms", "converged"}] * 3
    plain = pipeline.evaluate_clouds(pipeline.transform_cloud(reg["T"], moved), T, taus, voxel=v, crop=(lo, hi))
    assert {k: want[k] for k in want if k != "registration"} == plain       # key for key
    before = pipeline.evaluate_clouds(moved, T, taus, voxel=v, crop=(lo, hi))
    mid = len(taus) // 2
    print("F at tau", taus[mid], "unregistered", before["fscore"][mid], "registered", want["fscore"][mid])
    assert want["fscore"][mid] > before["fscore"][mid]
    # without a preparation: the whole clouds are registered
    P, G, _ = motion_case()
    e = pipeline.evaluate_clouds(P, G, [0.001, 0.002], register=0.15)
    assert e["registration"] == pipeline.register_clouds(P, G, 0.15) and e["precision"] == [1.0, 1.0]
    assert {k: e[k] for k in e if k != "registration"} == pipeline.evaluate_clouds(pipeline.transform_cloud(e["registration"]["T"], P), G,
                                                                                 [0.001, 0.002])
    # the table: the registration's four lines, then today's
    table = pipeline.format_cloud_eval(want)
    rows = table.split("\n")
    assert rows[0] == "registered: radii 8 0.5 0.0199999996, rms %.9g" % reg["stages"][-1]["rms"]
    assert rows[1:4] == ["T %.17g %.17g %.17g %.17g" % tuple(r) for r in reg["T"]]
    assert "\n".join(rows[4:]) == pipeline.format_cloud_eval(plain)
    assert [[float(x) for x in r.split()[1:]] for r in rows[1:4]] == reg["T"]     # %.17g round-trips a double
    box = [repr(x) for x in lo + hi]
    tail = ["--voxel", repr(v), "--crop"] + box + ["--cpu"] + register_flags()
    r = subprocess.run([sys.executable, "-m", "DPE_MVS.evaluate", recon, gt, "--tau"] + [repr(t) for t in taus] + tail +
                       ["--json", str(tmp_path / "py.json")], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=PKG), timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == table
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_eval"), recon, gt] + [repr(t) for t in taus] + tail +
                       ["--json", str(tmp_path / "c.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == table
    for name in ("py.json", "c.json"):
        got = json.load(open(tmp_path / name))
        assert got.pop("n_tau") == len(taus) and got == want


def test_evaluation_without_the_option_is_unchanged(tmp_path):
    """Without `register` the dict has no new key and the tables of the existing cases are format_cloud_eval's of such a
    dict, byte for byte."""
    recon, gt, taus, v, lo, hi, want = prepared_files(tmp_path)
    assert "registration" not in want and "registered" not in pipeline.format_cloud_eval(want)
    assert pipeline.format_cloud_eval(want).startswith("prepared: voxel 0.00249999994")
    box = [repr(x) for x in lo + hi]
    for tail, e in ((["--voxel", repr(v), "--crop"] + box, want),
                    ([], pipeline.evaluate_clouds(*cloud_case("line")[:2], taus))):
        assert "registration" not in e
        r = subprocess.run([os.path.join(PKG, "bin", "dpe_eval"), recon, gt] + [repr(t) for t in taus] + tail + ["--cpu"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == pipeline.format_cloud_eval(e)
        r = subprocess.run([sys.executable, "-m", "DPE_MVS.evaluate", recon, gt, "--tau"] + [repr(t) for t in taus] + tail + ["--cpu"],
                           capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=PKG), timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == pipeline.format_cloud_eval(e)


def test_register_command_lines(tmp_path):
    P, G, _ = motion_case()
    col = np.random.default_rng(8).integers(0, 256, P.shape).astype(np.uint8)
    write_ply(tmp_path / "src.ply", P, col)
    write_ply(tmp_path / "tgt.ply", G)
    want = pipeline.register_clouds(P, G, [0.3, 0.05])
    from DPE_MVS import register
    text = register.format_registration(want, len(P))
    args = [str(tmp_path / "src.ply"), str(tmp_path / "tgt.ply")]
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_register")] + args + [str(tmp_path / "c.ply"), "0.3", "0.05", "--cpu"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == text
    r = subprocess.run([sys.executable, "-m", "DPE_MVS.register"] + args + [str(tmp_path / "py.ply"), "0.3", "0.05", "--cpu"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=PKG), timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == text
    assert open(tmp_path / "py.ply", "rb").read() == open(tmp_path / "c.ply", "rb").read()
    xyz, bgr = pipeline.read_point_cloud_colors(str(tmp_path / "c.ply"))
    assert same_bits(xyz, pipeline.transform_cloud(want["T"], P)) and same_bits(bgr, col)               # colours kept
    assert np.abs(xyz.astype(np.float64) - G[motion_case()[2]]).max() < 1e-6                            # and the source is home
    init = [repr(float(x)) for row in want["T"] for x in row]
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_register")] + args + [str(tmp_path / "i.ply"), "0.05", "--iters", "5", "--init"] +
                       init + ["--cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "2 steps" in r.stdout and "converged 2" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_register"), str(tmp_path / "none.ply"), args[1], str(tmp_path / "x.ply"), "0.1", "--cpu"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot read" in r.stderr


# ------------------------------------------------------------------------------ 7. ASan + UBSan
@pytest.mark.timeout(600)
def test_host_registration_under_asan_ubsan():
    """A stand-alone program (tests/sanitize/register_sanitize.cpp, linked with host/cloud_register.cpp,
    host/cloud_eval.cpp and host/ply_read.cpp only) runs the step at n = 1, 257 and 65 537 against a literal tree, the
    loop on the sheet of test_loop_recovers_a_known_motion and the refusals; any report aborts it."""
    r = subprocess.run(["make", "-s", "sanitize-register"], cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(PKG, "bin", "register_sanitize")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "register sanitize ok" in r.stdout, r.stdout + r.stderr[-2000:]
