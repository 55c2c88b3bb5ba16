"""Depth-map evaluation on the host (host/depth_eval.cpp over csrc/depth_eval.h; include/dpe_mvs.h states the contract
of dpe_cloud_render_view and dpe_depth_score): the render of a scan into a view and the score of a map are pinned to
numpy references written from the contract's text (float32 elementwise operations in the stated order, np.minimum.at
for the z-buffer, s[0::2] + s[1::2] for the pairwise tree); the synthetic scene's own ground truth must score as the
contract predicts; the folder tool's two programs must print the same bytes; every refusal must come with a message;
and a stand-alone ASan + UBSan program walks the same ground.  The device path is compared with this one in
tests/test_depth_eval_gpu.py, which shares the cases below."""
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

F = np.float32
U = np.uint32
EMPTY = U(0x7F800000)
SIZES = [(1, 1), (7, 5), (65, 33)]
SPLATS = [0, 1, 2, 8]
COUNTS = [0, 1, 63, 64, 65, 257, 4097]
SCORE_SIZES = [(1, 1), (255, 1), (16, 16), (257, 1), (65537, 1)]       # w * h = 1, 255, 256, 257, 65 537


# ------------------------------------------------------------------------------ the numpy references
def usable(v):
    """positive and finite, on the bit pattern"""
    b = np.ascontiguousarray(v, F).view(U)
    return (b > 0) & (b < EMPTY)


def ref_render(pts, cam, s):
    w, h = int(cam.width), int(cam.height)
    p = np.ascontiguousarray(pts, F).reshape(-1, 3)
    R, t, K = (np.array(list(v), F) for v in (cam.R, cam.t, cam.K))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    finite = ((p.view(U) & EMPTY) != EMPTY).all(axis=1)
    with np.errstate(all="ignore"):
        tx = R[0] * x + R[1] * y + R[2] * z + t[0]
        ty = R[3] * x + R[4] * y + R[5] * z + t[1]
        tz = R[6] * x + R[7] * y + R[8] * z + t[2]
        d = K[6] * tx + K[7] * ty + K[8] * tz
        px = (K[0] * tx + K[1] * ty + K[2] * tz) / d
        py = (K[3] * tx + K[4] * ty + K[5] * tz) / d
        fx, fy = px + F(0.5), py + F(0.5)
        keep = finite & usable(d) & (fx > F(-1)) & (fx < F(w)) & (fy > F(-1)) & (fy < F(h))
    for a in (tx, ty, tz, d, px, py, fx, fy):
        assert a.dtype == F
    cx, cy, bits = np.trunc(fx[keep]).astype(np.int64), np.trunc(fy[keep]).astype(np.int64), d[keep].view(U)
    zb = np.full(w * h, EMPTY, U)
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            xx, yy = cx + dx, cy + dy
            m = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            np.minimum.at(zb, yy[m] * w + xx[m], bits[m])
    return np.where(zb == EMPTY, U(0), zb).view(F).reshape(h, w)


def ref_tree(terms):
    s = np.asarray(terms, np.float64)
    while len(s) > 1:
        if len(s) & 1:
            s = np.concatenate([s, [0.0]])
        s = s[0::2] + s[1::2]
    return s[0]


def ref_score(est, gt, taus, relative):
    e_, g = np.ascontiguousarray(est, F).ravel(), np.ascontiguousarray(gt, F).ravel()
    gt_ok, est_ok = usable(g), usable(e_)
    both = gt_ok & est_ok
    with np.errstate(all="ignore"):
        e = np.abs(e_ - g)
        rel = e / g
        within = [int((both & (e < (F(t) * g if relative else F(t)))).sum()) for t in taus]
    assert e.dtype == F and rel.dtype == F
    e64, r64 = np.where(both, e.astype(np.float64), 0.0), np.where(both, rel.astype(np.float64), 0.0)
    err = np.where(both, e, np.where(gt_ok, F(-1), F(-2))).astype(F).reshape(np.shape(est))
    d = dict(n_px=g.size, n_gt=int(gt_ok.sum()), n_est=int(est_ok.sum()), n_both=int(both.sum()), within=within,
             sum_abs=ref_tree(e64), sum_rel=ref_tree(r64), sum_sq=ref_tree(e64 * e64))
    return d, err


COUNT_KEYS = ("n_px", "n_gt", "n_est", "n_both", "within")


def sums_of(d):
    return np.array([d["sum_abs"], d["sum_rel"], d["sum_sq"]], np.float64)


def same_score(a, b):
    return all(a[k] == b[k] for k in COUNT_KEYS) and same_bits(sums_of(a), sums_of(b))


# ------------------------------------------------------------------------------ the render cases (shared with the GPU file)
def pixel_camera(w, h):
    """K = R = identity, t = 0: the point (px * z, py * z, z) projects to (px, py) at depth z exactly when z is a power
    of two."""
    return synthetic.make_camera(np.eye(3), np.eye(3), np.zeros(3), w, h, 0.1, 100.0)


def rotated_camera(w, h, offset):
    """a rotated R and a centre `offset` away on every axis"""
    a, b = 0.3, -0.2
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    R = Rx @ Ry
    C = np.array([offset, -offset, offset], np.float64)
    K = np.array([[1.2 * w, 0, w / 2.0], [0, 1.2 * w, h / 2.0], [0, 0, 1.0]])
    return synthetic.make_camera(K, R, -R @ C, w, h, 0.1, 100.0), K, R, C


def scattered_cloud(n, w, h, seed, offset=1000.0):
    """n points in front of rotated_camera(w, h, offset), some of them off every border, on a few depths so that pixels
    are shared and depths tie; from 64 points on also points that render nothing"""
    cam, K, R, C = rotated_camera(w, h, offset)
    rng = np.random.default_rng(seed)
    px, py = rng.uniform(-4, w + 4, n), rng.uniform(-4, h + 4, n)
    z = rng.choice([1.5, 2.0, 2.0, 3.25, 7.0], n) + rng.choice([0.0, 0.0, 1e-3], n)
    rays = np.stack([px, py, np.ones(n)], -1) @ np.linalg.inv(K).T
    pts = (C + z[:, None] * (rays @ R)).astype(F)
    if n >= 64:
        pts[3] = (C - 2.0 * R[2]).astype(F)                      # behind the camera
        pts[5] = C.astype(F)                                    # at the centre, as well as float32 can say
        pts[7] = (F(3e38), F(3e38), F(3e38))                    # finite coordinates whose depth overflows
        pts[11], pts[13], pts[17] = (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)   # a non-finite coordinate in each position
        pts[19] = (np.nan, np.nan, np.nan)
    return pts, cam


def border_cloud(w, h):
    """Through pixel_camera: fx and fy at -1, at the first float past it that a px + 0.5f can give, at the last float
    below w (h) and at w (h) itself, each at a depth of its own; points whose splat crosses each border and each corner;
    z = 0, a negative z, depths of +inf and NaN; two points on one pixel with equal z, and a nearer and a farther one."""
    lo = [F(-1.5), np.nextafter(F(-1.5), F(0)), np.nextafter(F(-1.5), F(-9))]
    pts, z = [], F(0.5)

    def add(px, py, depth=None):
        nonlocal z
        d = z if depth is None else F(depth)
        pts.append((F(px) * d, F(py) * d, d))
        z = z * F(2) if z < F(64) else F(0.5)
    for size, axis in ((w, 0), (h, 1)):
        hi = [F(size - 0.5), F(np.float64(np.nextafter(F(size), F(0))) - 0.5), np.nextafter(F(size - 0.5), F(0)), np.nextafter(F(size - 0.5), F(1e9))]
        for v in lo + hi:
            add(*((v, F(0)) if axis == 0 else (F(0), v)))
    for px in (0, (w - 1) / 2.0, w - 1):                             # borders and corners, for every splat
        for py in (0, (h - 1) / 2.0, h - 1):
            add(np.floor(px), np.floor(py), 4.0)
    add(-0.75, -0.75, 2.0)                                          # fx in (-1, 0): truncates to pixel 0
    mid = (F(w // 2), F(h // 2))
    add(*mid, 8.0), add(*mid, 8.0), add(*mid, 4.0), add(*mid, 16.0)
    pts += [(0, 0, 0), (0, 0, -1), (F(1e38), 0, F(3e38)), (0, 0, np.inf), (np.nan, 0, 1), (0, np.nan, 1), (0, 0, np.nan)]
    return np.array(pts, F), pixel_camera(w, h)


def one_pixel_cloud(n=20000):
    """n points on one pixel of a 7 x 5 image, their depths a permutation with the minimum somewhere in the middle"""
    d = np.random.default_rng(2).permutation(n).astype(F) * F(2 ** -10) + F(1)
    return np.stack([F(3) * d, F(2) * d, d], -1).astype(F), pixel_camera(7, 5)


@functools.lru_cache(maxsize=None)
def render_case(name):
    """(points, camera, splat, the numpy reference's map), computed once"""
    kind, *a = name.split("-")
    if kind == "scatter":
        w, h, s, n = map(int, a)
        pts, cam = scattered_cloud(n, w, h, seed=100 + n)
    elif kind == "border":
        w, h, s = map(int, a)
        pts, cam = border_cloud(w, h)
    elif kind == "onepixel":
        s = int(a[0])
        pts, cam = one_pixel_cloud()
    elif kind == "empty":                                           # a cloud that misses the image altogether
        s = 2
        pts, cam = scattered_cloud(257, 7, 5, seed=9)
        cam = rotated_camera(7, 5, -1000.0)[0]
    elif kind == "near":                                            # the camera's centre at -1000 on every axis instead of +1000
        s = 1
        pts, cam = scattered_cloud(4097, 65, 33, seed=4, offset=-1000.0)
    pts.setflags(write=False)
    return pts, cam, s, ref_render(pts, cam, s)


RENDER_CASES = (["scatter-%d-%d-%d-%d" % (w, h, s, n) for (w, h) in SIZES for s in SPLATS for n in COUNTS] +
                ["border-%d-%d-%d" % (w, h, s) for (w, h) in SIZES for s in SPLATS] +
                ["onepixel-0", "onepixel-1", "empty", "near"])


# ------------------------------------------------------------------------------ the score cases (shared with the GPU file)
TAUS = [0.0, 0.125, 0.5, 2.0]


def error_pair(tau, relative, side):
    """(est, gt) whose error |est - gt| is exactly tau (relative: tau * gt as the contract rounds it) for side 0, the
    float below it for side -1, the float above it for side +1.  est - gt is exact for neighbours, so the pair is
    searched among ground truths small or coarse enough for est = gt + e to be a float."""
    rng = np.random.default_rng(5)
    G = np.concatenate([F(2.0) ** -np.arange(0, 41, dtype=F), (rng.integers(2 ** 22, 2 ** 23, 4096) * 2.0 ** -22).astype(F)])
    t = F(tau) * G if relative else np.full(len(G), F(tau))
    e = t if side == 0 else np.nextafter(t, F(side * np.inf))
    est = G + e
    ok = (np.abs(est - G) == e) & usable(est) & usable(G)
    assert ok.any(), (tau, relative, side)
    i = int(np.argmax(ok))
    return est[i], G[i]


EDGE_TAUS = {False: (0.125, 0.5), True: (2.0,)}                     # the thresholds with pixels one ulp either side


def score_maps(w, h, relative, seed):
    """est and gt with every kind of unusable value, and with errors at tau (relative: tau * gt) and one ulp either side"""
    rng = np.random.default_rng(seed)
    n = w * h
    gt = rng.choice([1.0, 2.0, 4.0, 3.0], n).astype(F)
    est = (gt + rng.normal(0, 0.3, n)).astype(F)
    at = 0
    for tau in EDGE_TAUS[relative]:
        for side in (-1, 0, 1):
            est[at % n], gt[at % n] = error_pair(tau, relative, side)
            at += 1
    bad = [0.0, -0.0, -1.0, np.inf, -np.inf, np.nan]
    for j, v in enumerate(bad):
        if n > 40:
            est[20 + j] = v
            gt[30 + j] = v
    if n > 50:
        est[40], gt[40] = np.nan, np.inf                            # both unusable
        est[41], gt[41] = F(2.0), F(2.0)                            # an exact hit: e = 0 is not < tau = 0
    return est.reshape(h, w), gt.reshape(h, w)


@functools.lru_cache(maxsize=None)
def score_case(name):
    """(est, gt, relative, the numpy reference's dict and error map)"""
    kind, w, h, mode = name.split("-")
    w, h, relative = int(w), int(h), mode == "rel"
    if kind == "mixed":
        est, gt = score_maps(w, h, relative, seed=w * h)
    else:                                                           # every pixel invalid one way or another
        gt = np.resize(np.array([0.0, -1.0, np.nan, np.inf, 2.0, -0.0], F), w * h).reshape(h, w)
        est = np.resize(np.array([1.0, 2.0, 3.0, 1.0, -2.0, np.nan], F), w * h).reshape(h, w)
    return (est, gt, relative) + ref_score(est, gt, TAUS, relative)


SCORE_CASES = ["%s-%d-%d-%s" % (k, w, h, m) for k in ("mixed", "invalid") for (w, h) in SCORE_SIZES for m in ("abs", "rel")]


# ------------------------------------------------------------------------------ 1. the render against numpy
@pytest.mark.parametrize("name", RENDER_CASES)
def test_host_render_matches_numpy(name):
    pts, cam, s, want = render_case(name)
    got = pipeline.render_cloud(pts, cam, s)
    assert same_bits(got, want), (name, int((got.view(U) != want.view(U)).sum()))


def test_render_cases_reach_what_they_claim():
    for (w, h) in SIZES:
        pts, cam = border_cloud(w, h)
        fx = pts[:7, 0] / pts[:7, 2] + F(0.5)
        assert F(-1) in fx and F(w) in fx and np.nextafter(F(w), F(0)) in fx and ((fx > F(-1)) & (fx < F(-0.99))).any()
        m = pipeline.render_cloud(pts, cam, 0)
        assert m[h // 2, w // 2] == F(4.0) or (w, h) == (1, 1)       # the nearer of four on one pixel (1 x 1: everything lands there)
        assert not np.isnan(m).any() and (m >= 0).all() and np.isfinite(m).all()
    assert (render_case("scatter-65-33-0-4097")[3] > 0).mean() > 0.5
    assert (render_case("near")[3] > 0).mean() > 0.5
    assert not render_case("empty")[3].any() and not render_case("scatter-7-5-1-0")[3].any()
    pts, cam, _, want = render_case("onepixel-0")
    assert np.count_nonzero(want) == 1 and want[2, 3] == pts[:, 2].min() == F(1.0)
    assert np.count_nonzero(render_case("onepixel-1")[3]) == 9
    big = render_case("border-7-5-8")[3]
    assert (big > 0).all()                                           # half-width 8 floods a 7 x 5 image


# ------------------------------------------------------------------------------ 2. the score against numpy
@pytest.mark.parametrize("name", SCORE_CASES)
def test_host_score_matches_numpy(name):
    est, gt, relative, want, want_err = score_case(name)
    got, err = pipeline.score_depth(est, gt, TAUS, relative, want_error=True)
    assert same_score(got, want), (got, want)
    assert same_bits(err, want_err)
    assert same_score(pipeline.score_depth(est, gt, TAUS, relative), want)
    if name.startswith("invalid"):
        assert got["n_both"] == 0 and got["within"] == [0] * 4
        assert same_bits(sums_of(got), np.zeros(3))                  # +0.0, not -0.0
        assert got["mae"] == got["rmse"] == 0.0 and got["accuracy"] == [0.0] * 4
        assert set(np.unique(err)) <= {F(-1), F(-2)}


def test_score_thresholds_are_strict_and_derived_numbers_follow():
    est, gt, _, want, err = score_case("mixed-257-1-abs")
    assert want["within"][0] == 0                                    # tau = 0: nothing is below it
    assert 0 < want["within"][1] < want["within"][2] < want["within"][3] <= want["n_both"] < want["n_gt"] < want["n_px"]
    e = np.abs(est.ravel() - gt.ravel())
    for tau in (F(0.125), F(0.5)):                                   # one ulp either side of tau, and tau itself
        assert (e == tau).any() and (e == np.nextafter(tau, F(0))).any() and (e == np.nextafter(tau, F(9))).any()
    r_est, r_gt, _, r_want, _ = score_case("mixed-257-1-rel")
    e, t = np.abs(r_est.ravel() - r_gt.ravel())[:3], (F(2.0) * r_gt.ravel())[:3]
    assert e[0] == np.nextafter(t[0], F(0)) and e[1] == t[1] and e[2] == np.nextafter(t[2], F(np.inf))   # and of tau * gt
    hits = ref_score(r_est.ravel()[:3].reshape(1, 3), r_gt.ravel()[:3].reshape(1, 3), TAUS, True)[0]["within"]
    assert hits[3] == 1                                              # only the one below tau * gt is within it
    got = pipeline.score_depth(est, gt, TAUS)
    nb = got["n_both"]
    assert got["accuracy"] == [w / nb for w in got["within"]] and got["completeness"] == [w / got["n_gt"] for w in got["within"]]
    assert got["mae"] == got["sum_abs"] / nb and got["mre"] == got["sum_rel"] / nb and got["rmse"] == np.sqrt(got["sum_sq"] / nb)
    assert abs(got["sum_abs"] - float(np.sum(np.where(err >= 0, err, 0), dtype=np.float64))) < 1e-9
    rel = pipeline.score_depth(est, gt, TAUS, relative=True)
    assert rel["within"] != got["within"] and same_bits(sums_of(rel), sums_of(got))   # the mode moves the counts alone


# ------------------------------------------------------------------------------ 3. the synthetic scene
@functools.lru_cache(maxsize=None)
def scene():
    sc = synthetic.make_scene(96, 72, 4)
    return sc, synthetic.gt_point_cloud(sc, 1)


def test_the_scene_scores_as_the_contract_predicts():
    """A numpy z-buffer written from the contract gave coverage 1.000 and 0.985 within 1e-2; the rest is the
    see-through at occlusion edges that the contract names."""
    sc, pts = scene()
    truth = sc["views"][0]["depth"].astype(F)
    rendered = pipeline.render_cloud(pts, sc["cams"][0], 0)
    s = pipeline.score_depth(truth, rendered, [1e-2, 1e-3], relative=True)
    print("coverage", s["n_gt"] / s["n_px"], "within 1e-2", s["completeness"][0])
    assert s["n_gt"] == s["n_px"] == 96 * 72                         # every ground-truth pixel covered
    assert s["completeness"][0] >= 0.97
    noisy = truth * (F(1) + F(0.01) * np.random.default_rng(1).standard_normal(truth.shape).astype(F))
    t = pipeline.score_depth(noisy, rendered, [1e-2, 1e-3], relative=True)
    assert t["n_both"] == s["n_both"] and t["accuracy"][1] < s["accuracy"][1]


# ------------------------------------------------------------------------------ 4. the folder tool
def depth_folder(tmp_path, w=64, h=48, views=3):
    """A dense folder whose maps the test writes: the scene's depth with noise as depth.npy, a thinned copy as
    depth_filtered.npy, the scene's own depth as ground-truth maps; the scan as a PLY."""
    d = str(tmp_path / "dense")
    sc = synthetic.write_dense_folder(d, w, h, views, with_edges=False)
    rng = np.random.default_rng(3)
    os.makedirs(tmp_path / "gtmaps", exist_ok=True)
    for i, v in enumerate(sc["views"]):
        rf = os.path.join(d, pipeline.OUT_NAME, "%08d" % i)
        os.makedirs(rf, exist_ok=True)
        est = (v["depth"] * (1 + 0.004 * rng.standard_normal(v["depth"].shape))).astype(F)
        np.save(os.path.join(rf, "depth.npy"), est)
        np.save(os.path.join(rf, "depth_filtered.npy"), np.where(rng.random(est.shape) < 0.7, est, F(0)).astype(F))
        np.save(str(tmp_path / "gtmaps" / ("%08d.npy" % i)), v["depth"].astype(F))
    os.makedirs(os.path.join(d, pipeline.OUT_NAME, "00000007"), exist_ok=True)   # a folder without the map is no image
    pts = synthetic.gt_point_cloud(sc, 1)
    write_ply(tmp_path / "gt.ply", pts)
    return d, str(tmp_path / "gt.ply"), str(tmp_path / "gtmaps"), sc


FOLDER_TAUS = [0.01, 0.05]


def run_cli(args, **kw):
    return subprocess.run([os.path.join(PKG, "bin", "dpe_depth_eval")] + args, capture_output=True, text=True, timeout=120, **kw)


def run_module(args):
    return subprocess.run([sys.executable, "-m", "DPE_MVS.depth_eval"] + args, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, PYTHONPATH=PKG))


def folder_variants(d, ply, maps, tmp_path):
    """(command-line tail, evaluate_depth_maps' keywords, whether a scan is given)"""
    return [([], {}, True), (["--relative", "--splat", "1"], dict(relative=True, splat=1), True),
            (["--map", "depth_filtered.npy"], dict(map_name="depth_filtered.npy"), True),
            (["--gt-maps", maps], dict(gt_maps=maps), False), (["--maps", "--relative"], dict(write_maps=True, relative=True), True)]


def test_folder_tool_programs_agree(tmp_path):
    d, ply, maps, sc = depth_folder(tmp_path)
    pts = pipeline.read_point_cloud(ply)
    taus = [repr(t) for t in FOLDER_TAUS]
    for tail, kw, scan in folder_variants(d, ply, maps, tmp_path):
        want = pipeline.evaluate_depth_maps(d, pts if scan else None, FOLDER_TAUS, **kw)
        text = pipeline.format_depth_eval(want)
        args = [d] + ([ply] if scan else []) + taus + tail + ["--cpu"]
        c = run_cli(args + ["--json", str(tmp_path / "c.json")])
        assert c.returncode == 0, c.stderr
        p = run_module(args + ["--json", str(tmp_path / "py.json")])
        assert p.returncode == 0, p.stderr
        assert c.stdout == p.stdout == text, (tail, c.stdout, text)
        assert [im["id"] for im in want["images"]] == [0, 1, 2] and len(text.splitlines()) == 2 + 3 + 1
        cj, pj = json.load(open(tmp_path / "c.json")), json.load(open(tmp_path / "py.json"))
        assert cj["total"] == pj["total"] == want["total"] and cj["images"] == pj["images"] and cj["tau"] == pj["tau"]
        # the total: integers add, doubles are added in ascending id
        tot = want["total"]
        assert tot["n_both"] == sum(im["n_both"] for im in want["images"]) and tot["within"] == [sum(im["within"][k] for im in want["images"]) for k in range(2)]
        acc = 0.0
        for im in want["images"]:
            acc = acc + im["sum_abs"]
        assert tot["sum_abs"] == acc
    # each image is render_cloud + score_depth of its map and camera
    one = pipeline.evaluate_depth_maps(d, pts, FOLDER_TAUS)["images"][1]
    est = np.load(os.path.join(d, pipeline.OUT_NAME, "00000001", "depth.npy"))
    assert same_bits(pipeline.read_npy_f32(os.path.join(d, pipeline.OUT_NAME, "00000001", "depth.npy")), est)
    gt = pipeline.render_cloud(pts, sc["cams"][1], 0)
    alone = pipeline.score_depth(est, gt, FOLDER_TAUS)
    assert same_score(one, alone) and one["completeness"][1] > 0.9
    # --maps wrote what was scored
    rf = os.path.join(d, pipeline.OUT_NAME, "00000001")
    assert same_bits(np.load(os.path.join(rf, "depth_gt.npy")), gt)
    assert same_bits(np.load(os.path.join(rf, "depth_error.npy")), pipeline.score_depth(est, gt, FOLDER_TAUS, want_error=True)[1])
    # against the scene's own maps the thinned map loses completeness, not accuracy: it keeps a random 70 % of pixels that
    # carry the same noise, so the two accuracies estimate one probability (about 0.95 here) from 6 000 and 9 000 samples,
    # a standard error of 0.003 each
    full, thin = (pipeline.evaluate_depth_maps(d, None, FOLDER_TAUS, gt_maps=maps, map_name=m)["total"] for m in ("depth.npy", "depth_filtered.npy"))
    assert thin["n_est"] < full["n_est"] and thin["completeness"][1] < 0.8 * full["completeness"][1] and abs(thin["accuracy"][1] - full["accuracy"][1]) < 0.02


def write_raw_npy(path, descr="'<f4'", order="False", shape="(2, 3)", body=b"\0" * 24, version=b"\x01\x00", head=None):
    head = head or "{'descr': %s, 'fortran_order': %s, 'shape': %s, }" % (descr, order, shape)
    head += " " * ((16 - (10 + len(head) + 1) % 16) % 16) + "\n"
    with open(path, "wb") as f:
        f.write(b"\x93NUMPY" + version + len(head).to_bytes(2, "little") + head.encode() + body)


def test_refusals_come_with_a_message(tmp_path):
    d, ply, maps, sc = depth_folder(tmp_path, 32, 24, 2)
    pts = pipeline.read_point_cloud(ply)
    cam = sc["cams"][0]

    def refused(message, fn, *a, **kw):
        with pytest.raises(pipeline.PipelineError, match=message):
            fn(*a, **kw)
    refused("no such map", pipeline.evaluate_depth_maps, d, pts, [0.1], map_name="depth_none.npy")
    refused("no DPE folder", pipeline.evaluate_depth_maps, str(tmp_path / "nowhere"), pts, [0.1])
    refused("a scan or a folder", pipeline.evaluate_depth_maps, d, None, [0.1])
    refused("1 to 16 thresholds", pipeline.evaluate_depth_maps, d, pts, [0.1] * 17)
    refused("1 to 16 thresholds", pipeline.score_depth, np.ones((2, 2), F), np.ones((2, 2), F), [0.1] * 17)
    refused("negative or not finite", pipeline.score_depth, np.ones((2, 2), F), np.ones((2, 2), F), [-0.1])
    refused("negative or not finite", pipeline.score_depth, np.ones((2, 2), F), np.ones((2, 2), F), [np.nan])
    refused("size mismatch", pipeline.score_depth, np.ones((2, 2), F), np.ones((2, 3), F), [0.1])
    refused("splat half-width must be 0 to 8", pipeline.render_cloud, pts, cam, 9)
    refused("splat half-width must be 0 to 8", pipeline.render_cloud, pts, cam, -1)
    refused("splat half-width must be 0 to 8", pipeline.evaluate_depth_maps, d, pts, [0.1], splat=9)
    bad = _abi.DpeCamera()
    refused("width and height", pipeline.render_cloud, pts, bad, 0)
    # a ground-truth map of another size
    np.save(os.path.join(maps, "00000001.npy"), np.ones((5, 5), F))
    refused("size mismatch", pipeline.evaluate_depth_maps, d, None, [0.1], gt_maps=maps)
    os.remove(os.path.join(maps, "00000001.npy"))
    refused("cannot read npy", pipeline.evaluate_depth_maps, d, None, [0.1], gt_maps=maps)
    # bad .npy files
    p = str(tmp_path / "x.npy")
    for message, kw in (("dtype", dict(descr="'<f8'", body=b"\0" * 48)), ("dtype", dict(descr="'>f4'")), ("dtype", dict(descr="'<i4'")),
                        ("Fortran", dict(order="True")), ("truncated", dict(body=b"\0" * 23)), ("longer", dict(body=b"\0" * 25)),
                        ("2-D", dict(shape="(6,)")), ("2-D", dict(shape="(1, 2, 3)")), ("2-D", dict(shape="(0, 3)", body=b"")),
                        ("2-D", dict(shape="(2, x)")), ("version", dict(version=b"\x02\x00")), ("malformed", dict(head="{'descr': '<f4', 'fortran_order': False, }"))):
        write_raw_npy(p, **kw)
        refused(message, pipeline.read_npy_f32, p)
    open(p, "wb").write(b"\x93NUMPY\x01\x00\xff\xff{")
    refused("truncated .npy header", pipeline.read_npy_f32, p)
    open(p, "wb").write(b"PK\x03\x04")
    refused("not a .npy", pipeline.read_npy_f32, p)
    write_raw_npy(p, body=np.arange(6, dtype=F).tobytes())
    assert same_bits(pipeline.read_npy_f32(p), np.arange(6, dtype=F).reshape(2, 3))
    rf = os.path.join(d, pipeline.OUT_NAME, "00000000")
    np.save(os.path.join(rf, "depth.npy"), np.ones((24, 32), np.float64))
    refused("dtype", pipeline.evaluate_depth_maps, d, pts, [0.1])
    # and the programs say so on stderr
    for args, code, message in (([d, ply, "0.1", "--cpu"], 1, "dtype"), ([d, ply, "0.1", "--splat", "9", "--cpu"], 1, "splat"),
                                ([d, ply] + ["0.1"] * 17 + ["--cpu"], 1, "1 to 16 thresholds"), ([d, ply, "0.1", "--map", "none.npy", "--cpu"], 1, "no such map"),
                                ([d, str(tmp_path / "none.ply"), "0.1", "--cpu"], 1, "cannot read")):
        for r in (run_cli(args), run_module(args)):
            assert r.returncode == code and message in r.stderr, (args, r.stderr)
    assert run_cli([d]).returncode == 2 and run_cli([d, ply, "0.1", "--what"]).returncode == 2


# ------------------------------------------------------------------------------ 5. sanitizers
def test_depth_eval_under_sanitizers():
    """A stand-alone program (tests/sanitize/depth_sanitize.cpp, linked with host/depth_eval.cpp, host/ply_read.cpp,
    host/hostio.cpp and host/jpeg.cpp only) renders and scores cases of the kinds above against loops of its own, reads
    good and bad .npy files, runs the folder tool on a folder it writes and walks the refusals; any report aborts it."""
    r = subprocess.run(["make", "-s", "sanitize-depth"], cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(PKG, "bin", "depth_sanitize")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "depth sanitize ok" in r.stdout, r.stdout + r.stderr[-2000:]
