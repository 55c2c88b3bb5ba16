"""Normal-map evaluation on the host (host/normal_eval.cpp over csrc/normal_eval.h; include/dpe_mvs.h states the contract
of dpe_cloud_normals, dpe_cloud_render_view_normals and dpe_normal_score): the point normals, the render with winners
and the score are pinned to numpy references written from the contract's text (int64 sums by brute force over all pairs,
the Jacobi restated operation by operation in float64, np.minimum.at on the 64-bit words, s[0::2] + s[1::2] for the
pairwise tree); the solve is checked against numpy.linalg.eigh; the synthetic scene's analytic normals must score as the
issue's condition demands; the folder tool's two programs must print the same bytes; every refusal must come with a
message; and a stand-alone ASan + UBSan program walks the same ground.  The device path is compared with this one in
tests/test_normal_eval_gpu.py, which shares the cases below."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from DPE_MVS import _abi, pipeline, synthetic
from test_cloud_eval import PKG, same_bits
from test_cloud_voxel import write_ply
from test_depth_eval import pixel_camera, ref_tree, render_case, usable, write_raw_npy

F = np.float32
U = np.uint32
D = np.float64
EMPTY = U(0x7F800000)
SWEEPS = 8


# ------------------------------------------------------------------------------ the numpy reference of the point normals
def finite_rows(P):
    return ((np.ascontiguousarray(P, F).view(U) & EMPTY) != EMPTY).all(axis=1)


def ref_sums(P, R):
    """the ten int64 sums per point, by brute force over all pairs"""
    P = np.ascontiguousarray(P, F).reshape(-1, 3)
    n = len(P)
    fin = finite_rows(P)
    R32 = F(R)
    R2 = R32 * R32
    S = D(32768.0) / D(R32)
    out = np.zeros((n, 10), np.int64)
    for i0 in range(0, n, 512):
        q = P[i0:i0 + 512]
        with np.errstate(all="ignore"):
            d = [q[:, None, a] - P[None, :, a] for a in range(3)]
            s = d[0] * d[0]
            s = s + d[1] * d[1]
            s = s + d[2] * d[2]
            assert s.dtype == F
            nb = (s < R2) & fin[None, :] & fin[i0:i0 + 512, None]
            k = [np.trunc(np.where(nb, x, F(0)).astype(D) * S).astype(np.int64) for x in d]
        out[i0:i0 + 512, 0] = nb.sum(axis=1)
        for a in range(3):
            out[i0:i0 + 512, 1 + a] = k[a].sum(axis=1)
        for c, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            out[i0:i0 + 512, 4 + c] = (k[a] * k[b]).sum(axis=1)
    return out


def ref_covariance(sums):
    s = sums.astype(D)
    cnt = s[:, 0]
    with np.errstate(all="ignore"):
        m = {(a, b): s[:, 4 + c] - (s[:, 1 + a] * s[:, 1 + b]) / cnt for c, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))}
    return m


def ref_rotate(A, V, p, q, r):
    """one rotation of the contract, on every point at once; a zero off-diagonal entry keeps everything"""
    key = lambda i, j: (min(i, j), max(i, j))  # noqa: E731
    app, aqq, apq, arp, arq = A[p, p], A[q, q], A[p, q], A[key(r, p)], A[key(r, q)]
    skip = apq == 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        mag = np.where(theta < 0.0, -theta, theta)
        t = 1.0 / (mag + np.sqrt(theta * theta + 1.0))
        t = np.where(theta < 0.0, -t, t)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        new = {(p, p): app - h, (q, q): aqq + h, (p, q): np.zeros_like(apq), key(r, p): c * arp - s * arq, key(r, q): s * arp + c * arq}
        for k_, v in new.items():
            A[k_] = np.where(skip, A[k_], v)
        for row in range(3):
            a, b = V[row][p], V[row][q]
            V[row][p] = np.where(skip, a, c * a - s * b)
            V[row][q] = np.where(skip, b, s * a + c * b)


def ref_solve(sums, min_nb):
    """(normals f32 [n, 3], the covariance entries, valid) from the ten sums"""
    n = len(sums)
    A = ref_covariance(sums)
    C0 = {k: v.copy() for k, v in A.items()}
    V = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    for _ in range(SWEEPS):
        ref_rotate(A, V, 0, 1, 2)
        ref_rotate(A, V, 0, 2, 1)
        ref_rotate(A, V, 1, 2, 0)
    e0, e1, e2 = A[0, 0], A[1, 1], A[2, 2]
    with np.errstate(all="ignore"):
        col = np.zeros(n, np.int64)
        e = e0.copy()
        take = e1 < e
        col[take], e[take] = 1, e1[take]
        take = e2 < e
        col[take], e[take] = 2, e2[take]
        lo01, hi01 = np.where(e0 < e1, e0, e1), np.where(e0 < e1, e1, e0)
        t = np.where(hi01 < e2, hi01, e2)
        mid = np.where(lo01 < t, t, lo01)
        valid = (sums[:, 0] >= min_nb) & (sums[:, 0] >= 1) & (mid > 0.0)
        x, y, z = (np.choose(col, [V[row][0], V[row][1], V[row][2]]) for row in range(3))
        length = np.sqrt((x * x + y * y) + z * z)
        x, y, z = x / length, y / length, z / length
        ax, ay, az = (np.where(v < 0.0, -v, v) for v in (x, y, z))
        lead, am = x.copy(), ax.copy()
        take = ay > am
        lead[take], am[take] = y[take], ay[take]
        take = az > am
        lead[take], am[take] = z[take], az[take]
        flip = lead < 0.0
        nrm = np.stack([np.where(flip, -v, v) for v in (x, y, z)], -1)
    nrm = np.where(valid[:, None], nrm, 0.0).astype(F)
    return nrm, C0, valid


# ------------------------------------------------------------------------------ the clouds (shared with the GPU file)
def plane_patch(offset):
    u, v = np.meshgrid(np.arange(16) * 0.01, np.arange(16) * 0.01)
    return np.stack([offset + u, -offset + v, offset + 0.5 * u - 0.25 * v], -1).reshape(-1, 3).astype(F)


def ulp_cloud():
    """neighbours whose d2 is exactly R2 (R = 0.5), the float below it and the float above it, on each axis and side"""
    below, at, above = np.nextafter(F(0.5), F(0)), F(0.5), np.nextafter(F(0.5), F(1))
    pts = [(0, 0, 0)]
    for a in range(3):
        for sign in (1, -1):
            for d in (below, at, above):
                p = [0, 0, 0]
                p[a] = sign * d
                pts.append(p)
    return np.array(pts, F)


def clustered(n, R, seed, per=6):
    """clusters of `per` points within half of R per axis of centres spread over the unit cube: a cluster lies across
    several cells, and the cloud occupies more cells than its grid has buckets"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, ((n + per - 1) // per, 3))
    return (np.repeat(centres, per, axis=0)[:n] + rng.uniform(-0.5 * R, 0.5 * R, (n, 3))).astype(F)


@functools.lru_cache(maxsize=None)
def normals_case(name):
    """(points, R, min_nb, the numpy reference's sums, normals, covariance and validity), computed once"""
    rng = np.random.default_rng(sum(map(ord, name)))
    R, min_nb = 0.3, 3
    if name in ("n1", "n2", "n3"):
        P = np.array([(0, 0, 0), (0.1, 0, 0), (0, 0.1, 0.05)], F)[:int(name[1])]
    elif name == "collinear-axis":
        P, R = np.stack([np.arange(64) * 0.01, np.full(64, 0.5), np.full(64, -0.25)], -1).astype(F), 0.05
    elif name == "collinear-diagonal":
        P, R = np.repeat(np.arange(64, dtype=F)[:, None] * F(0.0078125), 3, axis=1), 0.05
    elif name == "copies":
        P, R = np.tile(np.array([(1.5, -2.0, 3.0)], F), (1000, 1)), 0.1
    elif name in ("plane+1000", "plane-1000"):
        P, R, min_nb = plane_patch(1000.0 if "+" in name else -1000.0), 0.035, 6
    elif name == "nonfinite":
        P = rng.uniform(0, 1, (300, 3)).astype(F)
        P[3], P[50], P[51], P[299] = (np.nan, 0, 0), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (np.nan, np.nan, np.nan)
    elif name == "ulp":
        P, R = ulp_cloud(), 0.5
    elif name in ("n65", "n257"):
        P = rng.uniform(0, 1, (int(name[1:]), 3)).astype(F)
    elif name == "spread":
        P, R, min_nb = clustered(4100, 0.02, 7), 0.02, 5
    elif name == "onecell":
        P, R = rng.uniform(0, 0.2, (5000, 3)).astype(F), 1.0
    P.setflags(write=False)
    sums = ref_sums(P, R)
    nrm, C0, valid = ref_solve(sums, min_nb)
    return P, R, min_nb, sums, nrm, C0, valid


NORMALS_CASES = ["n1", "n2", "n3", "collinear-axis", "collinear-diagonal", "copies", "plane+1000", "plane-1000", "nonfinite", "ulp",
                 "n65", "n257", "spread", "onecell"]
# numpy.linalg.eigh against the Jacobi on the valid points of the clouds above whose two smallest eigenvalues are
# clearly apart: the largest angle measured on the CPU was 2.51e-6 degrees (4.4e-8 radians, the rounding of the
# components to float); ten times that is asserted
EIGH_MAX_DEG = 10 * 2.51e-6


def walk_buckets(P, R):
    """per finite point: how often a neighbour would be met by a walk that visits every in-range cell's bucket, cells
    that share a bucket included (the grid of csrc/cloud_dist.h restated); returns (occupied cells, buckets, visits
    per true neighbour pair summed over the cloud, the true neighbour pairs)"""
    P = np.ascontiguousarray(P, F)
    fin = finite_rows(P)
    Q = P[fin].astype(D)
    m = len(Q)
    h = max(D(F(R)), 2.0 ** -62) * (1.0 + 2.0 ** -10)
    o = Q.min(axis=0)
    cell = np.floor((Q - o) / h).astype(np.int64)
    top = np.floor((Q.max(axis=0) - o) / h).astype(np.int64)
    nb = 64
    while nb < (1 << 28) and nb * 4 < m:
        nb <<= 1

    def bucket(c):
        c = c.astype(np.int64) & 0xFFFFFFFF
        return (((c[..., 0] * 73856093) & 0xFFFFFFFF) ^ ((c[..., 1] * 19349663) & 0xFFFFFFFF) ^ ((c[..., 2] * 83492791) & 0xFFFFFFFF)) & (nb - 1)
    own = bucket(cell)
    offs = np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    around = cell[:, None, :] + offs[None]
    inside = ((around >= 0) & (around <= top)).all(axis=2)
    bk = np.where(inside, bucket(around), -1)                          # [m, 27]
    Pf = P[fin]
    R2 = F(R) * F(R)
    visits = pairs = 0
    for i0 in range(0, m, 512):
        q = Pf[i0:i0 + 512]
        d = [q[:, None, a] - Pf[None, :, a] for a in range(3)]
        s = d[0] * d[0]
        s = s + d[1] * d[1]
        s = s + d[2] * d[2]
        near = s < R2
        met = (bk[i0:i0 + 512, :, None] == own[None, None, :]).sum(axis=1)   # how many of the 27 visits reach each point's bucket
        visits += int((met * near).sum())
        pairs += int(near.sum())
    return len(np.unique(cell, axis=0)), nb, visits, pairs


# ------------------------------------------------------------------------------ 1. the point normals against numpy
@pytest.mark.parametrize("name", NORMALS_CASES)
def test_host_normals_match_numpy(name):
    P, R, min_nb, sums, want, _, valid = normals_case(name)
    got, counts, got_sums = pipeline.estimate_normals(P, R, min_nb, want_sums=True)
    assert np.array_equal(counts, sums[:, 0]) and np.array_equal(got_sums, sums), name   # the integers first
    assert same_bits(got, want), (name, int((got.view(U) != want.view(U)).any(axis=1).sum()))
    plain, c2 = pipeline.estimate_normals(P, R, min_nb)
    assert same_bits(plain, got) and np.array_equal(c2, counts)
    assert np.array_equal(got.any(axis=1), valid)
    length = np.sqrt((got.astype(D) ** 2).sum(axis=1))
    assert np.all((np.abs(length[valid] - 1) < 1e-6)) and not got[~valid].any()
    assert (got[valid].max(axis=1) == np.abs(got[valid]).max(axis=1)).all()                # the largest component is positive


def test_normals_cases_reach_what_they_claim():
    for name in ("n1", "n2"):
        assert not normals_case(name)[6].any()                          # below min_nb
    P, R, min_nb, sums, nrm, _, valid = normals_case("n3")
    assert valid.all() and list(sums[:, 0]) == [3, 3, 3]
    assert not normals_case("collinear-axis")[6].any() and normals_case("collinear-axis")[3][:, 0].min() >= 5
    sums, valid = normals_case("copies")[3], normals_case("copies")[6]
    assert (sums[:, 0] == 1000).all() and not sums[:, 1:].any() and not valid.any()
    for name in ("plane+1000", "plane-1000"):                           # the offset does not cancel: every point has the plane's normal
        P, R, min_nb, sums, nrm, _, valid = normals_case(name)
        assert valid.all()
        pn = np.array([-0.5, 0.25, 1.0]) / np.linalg.norm([-0.5, 0.25, 1.0])
        assert np.abs(nrm.astype(D) @ pn).min() > 0.999                  # the points sit on float32's lattice at 1000: 6e-5 of 0.01
    P, R, min_nb, sums, nrm, _, valid = normals_case("nonfinite")
    assert not sums[[3, 50, 51, 299]].any() and not nrm[[3, 50, 51, 299]].any() and valid.sum() > 200
    sums = normals_case("ulp")[3]
    assert sums[0, 0] == 1 + 6                                          # itself and the six one ulp inside R; at R and beyond: none
    occupied, buckets, visits, pairs = walk_buckets(*normals_case("spread")[:2])
    print("spread: occupied cells", occupied, "buckets", buckets, "visits", visits, "pairs", pairs)
    assert occupied > buckets and visits > pairs                         # a walk that reads a shared bucket twice counts too many
    counts = normals_case("spread")[3][:, 0]
    assert counts.mean() > 4 and normals_case("spread")[6].sum() > 1000  # the clusters are neighbourhoods, and many give a normal
    sums = normals_case("onecell")[3]
    assert (sums[:, 0] == 5000).all() and sums[:, 4].max() > 2 ** 36     # large sums


def test_the_solve_agrees_with_eigh():
    worst = 0.0
    for name in NORMALS_CASES:
        P, R, min_nb, sums, nrm, C0, valid = normals_case(name)
        if not valid.any():
            continue
        M = np.zeros((len(P), 3, 3))
        for (a, b), v in C0.items():
            M[:, a, b] = M[:, b, a] = v
        w, vec = np.linalg.eigh(M[valid])
        apart = (w[:, 1] - w[:, 0]) > 1e-6 * w[:, 2]                    # a repeated smallest eigenvalue has no one eigenvector
        got = nrm[valid].astype(D)
        sin, cos = np.linalg.norm(np.cross(vec[:, :, 0], got), axis=1)[apart], np.abs((vec[:, :, 0] * got).sum(axis=1))[apart]
        if len(sin):                                                     # atan2 of the cross product: an arccos near 1 measures nothing
            worst = max(worst, float(np.degrees(np.arctan2(sin, cos)).max()))
    print("largest angle between the Jacobi's and eigh's eigenvector, degrees:", worst)
    assert worst <= EIGH_MAX_DEG


# ------------------------------------------------------------------------------ 2. the render with winners
def ref_render_normals(pts, normals, cam, s):
    """(depth map, normal map) from the contract's text: np.minimum.at on the words bits(z) << 32 | index"""
    w, h = int(cam.width), int(cam.height)
    p = np.ascontiguousarray(pts, F).reshape(-1, 3)
    nm = np.ascontiguousarray(normals, F).reshape(-1, 3)
    R, t, K = (np.array(list(v), F) for v in (cam.R, cam.t, cam.K))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    finite = finite_rows(p) if len(p) else np.zeros(0, bool)
    with np.errstate(all="ignore"):
        tx = R[0] * x + R[1] * y + R[2] * z + t[0]
        ty = R[3] * x + R[4] * y + R[5] * z + t[1]
        tz = R[6] * x + R[7] * y + R[8] * z + t[2]
        d = K[6] * tx + K[7] * ty + K[8] * tz
        px = (K[0] * tx + K[1] * ty + K[2] * tz) / d
        py = (K[3] * tx + K[4] * ty + K[5] * tz) / d
        fx, fy = px + F(0.5), py + F(0.5)
        keep = finite & usable(d) & (fx > F(-1)) & (fx < F(w)) & (fy > F(-1)) & (fy < F(h))
        ncx = R[0] * nm[:, 0] + R[1] * nm[:, 1] + R[2] * nm[:, 2]
        ncy = R[3] * nm[:, 0] + R[4] * nm[:, 1] + R[5] * nm[:, 2]
        ncz = R[6] * nm[:, 0] + R[7] * nm[:, 1] + R[8] * nm[:, 2]
        sgn = (ncx * tx + ncy * ty) + ncz * tz
    assert sgn.dtype == F
    idx = np.nonzero(keep)[0]
    cx, cy = np.trunc(fx[keep]).astype(np.int64), np.trunc(fy[keep]).astype(np.int64)
    word = (d[keep].view(U).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    empty = (np.uint64(EMPTY) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
    zb = np.full(w * h, empty, np.uint64)
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            xx, yy = cx + dx, cy + dy
            m = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            np.minimum.at(zb, yy[m] * w + xx[m], word[m])
    zbits = (zb >> np.uint64(32)).astype(U)
    covered = zbits != EMPTY
    depth = np.where(covered, zbits, U(0)).view(F).reshape(h, w)
    win = (zb & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out = np.zeros((w * h, 3), F)
    if len(p):
        j = np.where(covered, win, 0)
        has = covered & ((nm[j].view(U) & U(0x7FFFFFFF)) != 0).any(axis=1)
        out[has] = np.where((sgn[j] > F(0))[:, None], -nm[j], nm[j])[has]
    return depth, out.reshape(h, w, 3), np.where(covered, win, -1).reshape(h, w)


def normals_for(n, seed):
    """unit normals for n points, every fifth one missing"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v = (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9)).astype(F)
    v[::5] = 0
    if n > 7:
        v[7] = (-0.0, 0.0, -0.0)                                       # zeros of either sign are "no normal"
    return v


def special_cloud():
    """through pixel_camera(7, 5): pixel (1, 1) two points of equal depth with different normals; pixel (3, 2) a winner
    without a normal in front of a farther point with one; pixel (5, 3) a normal that must be flipped, pixel (5, 1) one
    that must not; pixel (0, 4) a far point alone"""
    pts = [(2, 2, 2), (2, 2, 2), (3, 2, 1), (12, 8, 4), (10, 6, 2), (10, 2, 2), (0, 16, 4)]
    nrm = [(1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 0, -1), (0.6, 0, 0.8), (0, 0.6, -0.8), (0, -1, 0)]
    return np.array(pts, F), np.array(nrm, F), pixel_camera(7, 5)


@functools.lru_cache(maxsize=None)
def render_normals_case(name):
    """(points, normals, camera, splat, the numpy reference's depth map, normal map and winners)"""
    if name.startswith("special"):
        pts, nrm, cam = special_cloud()
        s = int(name.split("-")[1])
    else:
        pts, cam, s, _ = render_case(name)
        nrm = normals_for(len(pts), 11)
    nrm.setflags(write=False)
    return (pts, nrm, cam, s) + ref_render_normals(pts, nrm, cam, s)


RENDER_NORMALS_CASES = ["special-0", "special-1", "scatter-65-33-1-4097", "scatter-65-33-0-257", "scatter-7-5-2-4097", "scatter-7-5-2-65",
                        "scatter-1-1-0-65", "scatter-1-1-2-1", "scatter-7-5-1-0", "border-7-5-2", "onepixel-0", "empty", "near"]


@pytest.mark.parametrize("name", RENDER_NORMALS_CASES)
def test_host_render_with_normals_matches_numpy(name):
    pts, nrm, cam, s, want_depth, want_normal, _ = render_normals_case(name)
    depth, normal = pipeline.render_cloud_normals(pts, nrm, cam, s)
    assert same_bits(depth, want_depth) and same_bits(depth, pipeline.render_cloud(pts, cam, s))   # render_cloud's bits
    assert same_bits(normal, want_normal), (name, int((normal.view(U) != want_normal.view(U)).any(axis=2).sum()))


def test_render_cases_reach_what_they_claim():
    pts, nrm, cam, s, depth, normal, win = render_normals_case("special-0")
    assert win[1, 1] == 0 and tuple(normal[1, 1]) == (-1, 0, 0)          # equal depth: the lower index wins (and faces the camera)
    assert win[2, 3] == 2 and depth[2, 3] == 1 and not normal[2, 3].any()   # the winner decides: the farther point is not consulted
    assert tuple(normal[3, 5]) == (F(-0.6), 0, F(-0.8)) and tuple(normal[1, 5]) == (0, F(0.6), F(-0.8))   # flipped / kept
    assert win[4, 0] == 6 and tuple(normal[4, 0]) == (0, -1, 0) and win[0, 0] == -1 and not normal[0, 0].any()
    assert (render_normals_case("special-1")[6] >= 0).sum() >= 30          # half-width 1 covers most of the 7 x 5 image
    pts, nrm, cam, s, depth, normal, win = render_normals_case("scatter-65-33-1-4097")
    has = normal.any(axis=2)
    assert 0.5 < has.mean() < (win >= 0).mean()                          # some winners have no normal
    R = np.array(list(cam.R), D).reshape(3, 3)
    C = -R.T @ np.array(list(cam.t), D)
    view = pts[win[has]].astype(D) - C                                   # from the camera to the winning point
    assert ((normal[has].astype(D) * view).sum(axis=1) <= 1e-3).all()    # every rendered normal faces the camera
    assert not render_normals_case("empty")[5].any() and not render_normals_case("scatter-7-5-1-0")[5].any()
    tie = render_normals_case("onepixel-0")
    assert tie[6][2, 3] == int(np.argmin(tie[0][:, 2]))


# ------------------------------------------------------------------------------ 3. the score against numpy
TAUS_DEG = [11.25, 30.0, 90.0, 180.0]
SCORE_SIZES = [(1, 1), (255, 1), (16, 16), (257, 1), (65537, 1)]       # w * h = 1, 255, 256, 257, 65 537
EDGE_BINS = (1, 45, 179)


def cos_taus():
    return np.array([pipeline.normal_cos(v) for v in TAUS_DEG], F)


def ref_cosine(e, g):
    """(est_ok, gt_ok, both, the unclamped cosine) of maps [n, 3], in float32"""
    with np.errstate(all="ignore"):
        ee = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        den = ee * gg
        c = ((e[:, 0] * g[:, 0] + e[:, 1] * g[:, 1]) + e[:, 2] * g[:, 2]) / np.sqrt(den)
    assert c.dtype == F
    e_ok, g_ok = finite_rows(e) & usable(ee), finite_rows(g) & usable(gg)
    return e_ok, g_ok, e_ok & g_ok & usable(den), c


def ref_score(est, gt, cos_tau):
    e, g = np.ascontiguousarray(est, F).reshape(-1, 3), np.ascontiguousarray(gt, F).reshape(-1, 3)
    e_ok, g_ok, both, raw = ref_cosine(e, g)
    with np.errstate(all="ignore"):
        c = np.where(raw < F(-1), F(-1), np.where(raw > F(1), F(1), raw)).astype(F)
        E = np.cos(np.arange(180, dtype=D) * np.pi / 180).astype(F)
        bins = (c[:, None] < E[None, 1:]).sum(axis=1)
        within = [int((both & (c > F(t))).sum()) for t in cos_tau]
    d = np.where(both, 1.0 - c.astype(D), 0.0)
    err = np.where(both, c, np.where(g_ok, F(-2), F(-3))).astype(F).reshape(np.shape(est)[:2])
    score = dict(n_px=len(e), n_gt=int(g_ok.sum()), n_est=int(e_ok.sum()), n_both=int(both.sum()), within=within,
                 hist=[int(v) for v in np.bincount(bins[both], minlength=180)], sum_dist=ref_tree(d), sum_dist_sq=ref_tree(d * d))
    return score, err


COUNT_KEYS = ("n_px", "n_gt", "n_est", "n_both", "within", "hist")


def sums_of(d):
    return np.array([d["sum_dist"], d["sum_dist_sq"]], D)


def same_score(a, b):
    return all(a[k] == b[k] for k in COUNT_KEYS) and same_bits(sums_of(a), sums_of(b))


def cosine_pair(target, side):
    """(est, gt = (1, 0, 0)) whose computed cosine is exactly `target` (side 0), the float below (-1) or above (+1):
    est = (x, 1, 0) has c = x / sqrtf(x * x + 1), which steps through the floats around target as x does"""
    want = F(target) if side == 0 else np.nextafter(F(target), F(side * 2))
    x0 = D(target) / np.sqrt(max(1.0 - D(target) ** 2, 1e-30))
    x = F(x0)
    xs = [x]
    lo = hi = x
    for _ in range(4096):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        xs += [lo, hi]
    e = np.stack([np.array(xs, F), np.ones(len(xs), F), np.zeros(len(xs), F)], -1)
    g = np.tile(np.array([(1, 0, 0)], F), (len(xs), 1))
    _, _, both, c = ref_cosine(e, g)
    ok = both & (c == want)
    assert ok.any(), (target, side)
    return e[int(np.argmax(ok))], g[0]


@functools.lru_cache(maxsize=None)
def edge_pixels():
    """pixels with c at a threshold and one ulp above it, at E[b] and one ulp either side, and with a dot above 1"""
    E = pipeline.normal_edges()
    px = [cosine_pair(cos_taus()[0], 0), cosine_pair(cos_taus()[0], 1), cosine_pair(cos_taus()[1], 0), cosine_pair(cos_taus()[1], 1)]
    for b in EDGE_BINS:
        px += [cosine_pair(E[b], side) for side in (-1, 0, 1)]
    rng = np.random.default_rng(8)
    v = rng.uniform(-2, 2, (65536, 3)).astype(F)
    k = (v * rng.uniform(0.5, 3, (65536, 1)).astype(F)).astype(F)
    _, _, both, c = ref_cosine(v, k)
    over = both & (c > F(1))
    assert over.any()                                                   # two parallel vectors: a cosine above 1 before the clamp
    px.append((v[int(np.argmax(over))], k[int(np.argmax(over))]))
    return px


def score_maps(w, h, seed):
    """est and gt with every kind of pixel without a normal, and the edge pixels in front"""
    rng = np.random.default_rng(seed)
    n = w * h
    gt = rng.standard_normal((n, 3)).astype(F)
    est = (gt + rng.normal(0, 0.4, (n, 3))).astype(F)
    est[n // 2:] *= F(0.01)                                             # the vectors need not be unit
    for at, (e, g) in enumerate(edge_pixels()):
        est[at % n], gt[at % n] = e, g
    bad = [(0, 0, 0), (-0.0, 0, -0.0), (np.inf, 0, 0), (0, np.nan, 1), (1, 1, -np.inf), (1e20, 0, 0), (1e-30, 0, 0)]
    if n > 60:
        for j, v in enumerate(bad):
            est[20 + j] = v
            gt[30 + j] = v
        est[40], gt[40] = (np.nan, 0, 0), (0, 0, 0)                     # neither
        est[41], gt[41] = (3e15, 0, 0), (0, 3e15, 3e15)                 # each usable, their product overflows
        est[42], gt[42] = (1e-12, 0, 0), (1e-12, 1e-12, 0)              # each usable, their product underflows to 0
        est[43], gt[43] = (0, 0, 2), (0, 0, -3)                         # opposite: c = -1
    return est.reshape(h, w, 3), gt.reshape(h, w, 3)


@functools.lru_cache(maxsize=None)
def score_case(name):
    """(est, gt, the numpy reference's dict and error map)"""
    kind, w, h = name.split("-")
    w, h = int(w), int(h)
    if kind == "mixed":
        est, gt = score_maps(w, h, seed=w * h)
    elif kind == "plane":                                               # one plane: every pixel in one bin
        est, gt = np.tile(np.array([(0.6, 0, -0.8)], F), (h, w, 1)), np.tile(np.array([(0, 0, -1)], F), (h, w, 1))
    else:                                                               # every pixel without a normal one way or another
        gt = np.resize(np.array([(0, 0, 0), (np.nan, 0, 1), (1, 0, 0), (np.inf, 1, 1), (0, 1, 0), (-0.0, 0, 0)], F), (w * h, 3)).reshape(h, w, 3)
        est = np.resize(np.array([(1, 0, 0), (1, 1, 1), (0, -0.0, 0), (1, 0, 0), (0, 0, np.nan), (1, 2, 3)], F), (w * h, 3)).reshape(h, w, 3)
    return (est, gt) + ref_score(est, gt, cos_taus())


SCORE_CASES = ["%s-%d-%d" % (k, w, h) for k in ("mixed", "invalid") for (w, h) in SCORE_SIZES] + ["plane-257-1", "plane-96-72"]


@pytest.mark.parametrize("name", SCORE_CASES)
def test_host_score_matches_numpy(name):
    est, gt, want, want_err = score_case(name)
    got, err = pipeline.score_normals(est, gt, cos_taus=cos_taus(), want_error=True)
    assert same_score(got, want), (name, {k: (got[k], want[k]) for k in COUNT_KEYS if got[k] != want[k]}, sums_of(got), sums_of(want))
    assert same_bits(err, want_err)
    assert same_score(pipeline.score_normals(est, gt, taus_deg=TAUS_DEG), want)   # degrees become these cosines
    assert sum(got["hist"]) == got["n_both"]
    if name.startswith("invalid"):
        assert got["n_both"] == 0 and got["within"] == [0] * 4 and not any(got["hist"])
        assert same_bits(sums_of(got), np.zeros(2))                      # +0.0, not -0.0
        assert got["mean_cos_dist"] == got["median_deg"] == got["mean_deg"] == 0.0 and got["share"] == [0.0] * 4
        assert set(np.unique(err)) <= {F(-2), F(-3)}
    if name.startswith("plane"):
        assert got["hist"][36] == got["n_both"] == got["n_px"] and got["median_deg"] == 36.5 and got["within"] == [0, 0, got["n_px"], got["n_px"]]


def test_score_edges_are_strict_and_derived_numbers_follow():
    E = pipeline.normal_edges()
    assert same_bits(E, np.cos(np.arange(180, dtype=D) * np.pi / 180).astype(F)) and (np.diff(E) < 0).all()
    assert all(pipeline.normal_cos(b) == E[b] for b in range(180)) and pipeline.normal_cos(180.0) == -1.0
    px = edge_pixels()
    t = cos_taus()
    one = lambda e, g: ref_score(np.array(e, F).reshape(1, 1, 3), np.array(g, F).reshape(1, 1, 3), t)  # noqa: E731
    assert one(*px[0])[0]["within"][0] == 0 and one(*px[1])[0]["within"][0] == 1     # c == cos(tau) is not within; one ulp above is
    assert one(*px[2])[0]["within"][:2] == [0, 0] and one(*px[3])[0]["within"][:2] == [0, 1]
    for k, b in enumerate(EDGE_BINS):                                   # c < E[b]: bin b; c == E[b] and above: bin b - 1
        below, at, above = (int(np.argmax(one(*px[4 + 3 * k + j])[0]["hist"])) for j in range(3))
        assert (below, at, above) == (b, b - 1, b - 1), (b, below, at, above)
    s, err = one(*px[-1])
    assert s["hist"][0] == 1 and err[0, 0] == F(1) and same_bits(sums_of(s), np.zeros(2))   # clamped to 1: distance +0.0
    for e, g in px:                                                      # and the library agrees pixel by pixel
        e_, g_ = np.array(e, F).reshape(1, 1, 3), np.array(g, F).reshape(1, 1, 3)
        assert same_score(pipeline.score_normals(e_, g_, cos_taus=t), one(e, g)[0])
    est, gt, want, err = score_case("mixed-257-1")
    assert want["n_both"] < want["n_gt"] < want["n_px"] and want["n_both"] < want["n_est"] and want["hist"][179] >= 1
    assert 0 < want["within"][0] < want["within"][1] < want["within"][2] < want["within"][3] < want["n_both"]   # c = -1 is not above cos 180
    got = pipeline.score_normals(est, gt, cos_taus=t)
    nb = got["n_both"]
    assert got["share"] == [w / nb for w in got["within"]] and got["completeness"] == [w / got["n_gt"] for w in got["within"]]
    assert got["mean_cos_dist"] == got["sum_dist"] / nb
    mean = 0.0
    for b, v in enumerate(got["hist"]):
        mean = mean + v * (b + 0.5)
    assert got["mean_deg"] == mean / nb
    run = np.cumsum(got["hist"])
    assert got["median_deg"] == int(np.argmax(2 * run >= nb)) + 0.5
    angles = np.degrees(np.arccos(np.clip(err[err >= -1].astype(D), -1, 1)))
    assert abs(got["mean_deg"] - angles.mean()) < 0.51 and abs(got["median_deg"] - np.median(angles)) < 1.01   # to the histogram's 1 degree


# ------------------------------------------------------------------------------ 4. the synthetic scene, end to end
@functools.lru_cache(maxsize=None)
def scene():
    sc = synthetic.make_scene(96, 72, 5)
    pts = synthetic.gt_point_cloud(sc, 1)
    nrm, counts = pipeline.estimate_normals(pts, 0.07)                  # min_neighbours: the default, 3
    return sc, pts, nrm, counts


def test_the_scene_end_to_end():
    """The issue's condition on the 96 x 72, 5-view scene: normals of the scene's own scan with R = 0.07, rendered into
    view 0 with s = 0 and scored against the analytic normals.  More than 0.99 of the pixels must be `both` and more
    than 0.95 of those within 11.25 degrees.  This contract gave 6908 of 6912 pixels and 0.98350 on the CPU, the float64
    prototype's 6908 and 0.983; the median angle fell in the histogram's first bin and the mean was 0.759 degrees."""
    sc, pts, nrm, counts = scene()
    depth, normal = pipeline.render_cloud_normals(pts, nrm, sc["cams"][0], 0)
    truth = sc["views"][0]["normals"].astype(F)
    s = pipeline.score_normals(truth, normal, taus_deg=[11.25, 30.0])
    print("both", s["n_both"], "of", s["n_px"], "within 11.25 degrees", s["share"][0], "median", s["median_deg"], "mean", s["mean_deg"])
    assert s["n_px"] == 96 * 72
    assert s["n_both"] > 0.99 * s["n_px"]
    assert s["share"][0] > 0.95
    assert same_bits(depth, pipeline.render_cloud(pts, sc["cams"][0], 0))
    flipped = pipeline.score_normals(-truth, normal, taus_deg=[11.25])   # a wrong sign falls far below
    assert flipped["share"][0] < 0.01


# ------------------------------------------------------------------------------ 5. the folder tool
def normal_folder(tmp_path, w=64, h=48, views=3):
    """A dense folder whose maps the test writes: the scene's normals with noise as normal.npy (some pixels without one),
    the scene's own normals as ground-truth maps; the scan as a PLY."""
    d = str(tmp_path / "dense")
    sc = synthetic.write_dense_folder(d, w, h, views, with_edges=False)
    rng = np.random.default_rng(3)
    os.makedirs(tmp_path / "gtnormals", exist_ok=True)
    for i, v in enumerate(sc["views"]):
        rf = os.path.join(d, pipeline.OUT_NAME, "%08d" % i)
        os.makedirs(rf, exist_ok=True)
        est = (v["normals"] + 0.05 * rng.standard_normal(v["normals"].shape)).astype(F)
        est[rng.random(est.shape[:2]) < 0.1] = 0
        np.save(os.path.join(rf, "normal.npy"), est)
        np.save(str(tmp_path / "gtnormals" / ("%08d.npy" % i)), v["normals"].astype(F))
    os.makedirs(os.path.join(d, pipeline.OUT_NAME, "00000007"), exist_ok=True)   # a folder without the map is no image
    pts = synthetic.gt_point_cloud(sc, 1)
    write_ply(tmp_path / "gt.ply", pts)
    return d, str(tmp_path / "gt.ply"), str(tmp_path / "gtnormals"), sc


FOLDER_TAUS = [11.25, 30.0]
FOLDER_R = 0.1


def run_cli(args, **kw):
    return subprocess.run([os.path.join(PKG, "bin", "dpe_normal_eval")] + args, capture_output=True, text=True, timeout=120, **kw)


def run_module(args):
    return subprocess.run([sys.executable, "-m", "DPE_MVS.normal_eval"] + args, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, PYTHONPATH=PKG))


def test_folder_tool_programs_agree(tmp_path):
    d, ply, maps, sc = normal_folder(tmp_path)
    pts = pipeline.read_point_cloud(ply)
    taus = [repr(t) for t in FOLDER_TAUS]
    for tail, kw, scan in (([], {}, True), (["--splat", "1", "--min-neighbours", "5"], dict(splat=1, min_neighbours=5), True),
                           (["--gt-normals", maps], dict(gt_normals=maps), False), (["--maps"], dict(write_maps=True), True)):
        want = pipeline.evaluate_normal_maps(d, pts if scan else None, FOLDER_R if scan else None, FOLDER_TAUS, **kw)
        text = pipeline.format_normal_eval(want)
        args = [d] + ([ply, repr(FOLDER_R)] if scan else []) + taus + tail + ["--cpu"]
        c = run_cli(args + ["--json", str(tmp_path / "c.json")])
        assert c.returncode == 0, c.stderr
        p = run_module(args + ["--json", str(tmp_path / "py.json")])
        assert p.returncode == 0, p.stderr
        assert c.stdout == p.stdout == text, (tail, c.stdout, text)
        assert [im["id"] for im in want["images"]] == [0, 1, 2] and len(text.splitlines()) == 2 + 3 + 1
        cj, pj = json.load(open(tmp_path / "c.json")), json.load(open(tmp_path / "py.json"))
        assert cj["total"] == pj["total"] == want["total"] and cj["images"] == pj["images"] and cj["tau_deg"] == pj["tau_deg"]
        tot = want["total"]                                              # integers add, doubles are added in ascending id
        assert tot["n_both"] == sum(im["n_both"] for im in want["images"]) and tot["hist"] == [sum(im["hist"][b] for im in want["images"]) for b in range(180)]
        acc = 0.0
        for im in want["images"]:
            acc = acc + im["sum_dist"]
        assert tot["sum_dist"] == acc
    # each image is estimate_normals + render_cloud_normals + score_normals of its map and camera
    one = pipeline.evaluate_normal_maps(d, pts, FOLDER_R, FOLDER_TAUS)["images"][1]
    est = np.load(os.path.join(d, pipeline.OUT_NAME, "00000001", "normal.npy"))
    assert same_bits(pipeline.read_npy_f32x3(os.path.join(d, pipeline.OUT_NAME, "00000001", "normal.npy")), est)
    nrm, _ = pipeline.estimate_normals(pts, FOLDER_R)
    _, gt = pipeline.render_cloud_normals(pts, nrm, sc["cams"][1], 0)
    alone = pipeline.score_normals(est, gt, taus_deg=FOLDER_TAUS)
    assert same_score(one, alone) and one["share"][1] > 0.9
    rf = os.path.join(d, pipeline.OUT_NAME, "00000001")                  # --maps wrote what was scored
    assert same_bits(np.load(os.path.join(rf, "normal_gt.npy")), gt)
    assert same_bits(np.load(os.path.join(rf, "normal_error.npy")), pipeline.score_normals(est, gt, taus_deg=FOLDER_TAUS, want_error=True)[1])
    full = pipeline.evaluate_normal_maps(d, None, None, FOLDER_TAUS, gt_normals=maps)["total"]
    assert full["n_gt"] == full["n_px"] and 0.85 < full["n_both"] / full["n_px"] < 0.95 and full["share"][0] > 0.9


def test_refusals_come_with_a_message(tmp_path):
    d, ply, maps, sc = normal_folder(tmp_path, 32, 24, 2)
    pts = pipeline.read_point_cloud(ply)
    cam = sc["cams"][0]
    ones = np.ones((2, 2, 3), F)

    def refused(message, fn, *a, **kw):
        with pytest.raises(pipeline.PipelineError, match=message):
            fn(*a, **kw)
    refused("no DPE folder", pipeline.evaluate_normal_maps, str(tmp_path / "nowhere"), pts, 0.1, [10])
    refused("a scan or a folder", pipeline.evaluate_normal_maps, d, None, None, [10])
    refused("1 to 16 thresholds", pipeline.evaluate_normal_maps, d, pts, 0.1, [10] * 17)
    refused("radius is not a finite positive", pipeline.evaluate_normal_maps, d, pts, 0.0, [10])
    refused("at least 3 neighbours", pipeline.evaluate_normal_maps, d, pts, 0.1, [10], min_neighbours=2)
    refused("splat half-width must be 0 to 8", pipeline.evaluate_normal_maps, d, pts, 0.1, [10], splat=9)
    refused("radius is not a finite positive", pipeline.estimate_normals, pts, np.nan)
    refused("radius is not a finite positive", pipeline.estimate_normals, pts, -1.0)
    refused("at least 3 neighbours", pipeline.estimate_normals, pts, 0.1, 2)
    refused("radius too small", pipeline.estimate_normals, np.array([(0, 0, 0), (3e38, 0, 0)], F), 1e-30)
    refused("one normal per point", pipeline.render_cloud_normals, pts, pts[:5], cam)
    refused("splat half-width must be 0 to 8", pipeline.render_cloud_normals, pts, pts, cam, 9)
    refused("width and height", pipeline.render_cloud_normals, pts, pts, _abi.DpeCamera(), 0)
    refused("1 to 16 thresholds", pipeline.score_normals, ones, ones, cos_taus=[0.5] * 17)
    refused("not in \\[-1, 1\\]", pipeline.score_normals, ones, ones, cos_taus=[1.5])
    refused("not in \\[-1, 1\\]", pipeline.score_normals, ones, ones, cos_taus=[np.nan])
    refused("size mismatch", pipeline.score_normals, ones, np.ones((2, 3, 3), F), cos_taus=[0.5])
    refused("size mismatch", pipeline.score_normals, np.ones((2, 2), F), np.ones((2, 2), F), cos_taus=[0.5])
    refused("degrees or as cosines", pipeline.score_normals, ones, ones)
    np.save(os.path.join(maps, "00000001.npy"), np.ones((5, 5, 3), F))   # a ground-truth map of another size
    refused("size mismatch", pipeline.evaluate_normal_maps, d, None, None, [10], gt_normals=maps)
    os.remove(os.path.join(maps, "00000001.npy"))
    refused("cannot read npy", pipeline.evaluate_normal_maps, d, None, None, [10], gt_normals=maps)
    p = str(tmp_path / "x.npy")                                          # bad .npy files
    for message, kw in (("dtype", dict(descr="'<f8'", shape="(2, 1, 3)", body=b"\0" * 48)), ("Fortran", dict(order="True", shape="(2, 1, 3)")),
                        ("truncated", dict(shape="(2, 1, 3)", body=b"\0" * 23)), ("longer", dict(shape="(2, 1, 3)", body=b"\0" * 25)),
                        ("3-D", dict(shape="(2, 3)")), ("3-D", dict(shape="(1, 3, 2)")), ("3-D", dict(shape="(1, 2, 3, 1)")),
                        ("3-D", dict(shape="(0, 2, 3)", body=b"")), ("version", dict(shape="(2, 1, 3)", version=b"\x02\x00"))):
        write_raw_npy(p, **kw)
        refused(message, pipeline.read_npy_f32x3, p)
    write_raw_npy(p, shape="(2, 1, 3)", body=np.arange(6, dtype=F).tobytes())
    assert same_bits(pipeline.read_npy_f32x3(p), np.arange(6, dtype=F).reshape(2, 1, 3))
    refused("2-D", pipeline.read_npy_f32, p)                             # the 2-D reader's refusals stay
    rf = os.path.join(d, pipeline.OUT_NAME, "00000000")
    np.save(os.path.join(rf, "normal.npy"), np.ones((24, 32), F))
    refused("3-D", pipeline.evaluate_normal_maps, d, pts, 0.1, [10])
    for args, code, message in (([d, ply, "0.1", "10", "--cpu"], 1, "3-D"), ([d, ply, "0.1", "10", "--splat", "9", "--cpu"], 1, "splat"),
                                ([d, ply, "0.1"] + ["10"] * 17 + ["--cpu"], 1, "1 to 16 thresholds"), ([d, ply, "0", "10", "--cpu"], 1, "radius"),
                                ([d, ply, "0.1", "10", "--min-neighbours", "1", "--cpu"], 1, "at least 3 neighbours"),
                                ([d, str(tmp_path / "none.ply"), "0.1", "10", "--cpu"], 1, "cannot read")):
        for r in (run_cli(args), run_module(args)):
            assert r.returncode == code and message in r.stderr, (args, r.stderr)
    os.remove(os.path.join(rf, "normal.npy"))
    os.remove(os.path.join(d, pipeline.OUT_NAME, "00000001", "normal.npy"))
    refused("no such map", pipeline.evaluate_normal_maps, d, pts, 0.1, [10])
    assert run_cli([d]).returncode == 2 and run_cli([d, ply, "0.1", "10", "--what"]).returncode == 2


# ------------------------------------------------------------------------------ 6. sanitizers
def test_normal_eval_under_sanitizers():
    """A stand-alone program (tests/sanitize/normal_sanitize.cpp, linked with host/normal_eval.cpp, host/depth_eval.cpp,
    host/cloud_eval.cpp, host/ply_read.cpp, host/hostio.cpp and host/jpeg.cpp only) estimates normals, renders and scores
    cases of the kinds above against loops of its own, reads good and bad 3-D .npy files, runs the folder tool on a folder
    it writes and walks the refusals; any report aborts it."""
    r = subprocess.run(["make", "-s", "sanitize-normal"], cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(PKG, "bin", "normal_sanitize")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "normal sanitize ok" in r.stdout, r.stdout + r.stderr[-2000:]
