"""The clouds of the voxel down-sampling tests (tests/test_cloud_voxel.py on the host, tests/test_cloud_voxel_gpu.py
on the device) and the numpy reference both are held to, written from the contract's text (include/dpe_mvs.h,
dpe_cloud_voxel): double arithmetic, np.unique on the integer cells, np.add.at on uint64.  Imports no HIP library."""
import numpy as np

from test_cloud_eval import adversarial_cloud, line_cloud, nonfinite_cloud, random_cloud

F = np.float32


def clustered(seed, n):
    """A copy of test_cloud_eval_gpu.clustered (importing that module loads the HIP library): n points in 40 clusters
    of very different density over a 10 x 10 x 2 slab, 50 of them far outliers."""
    rng = np.random.default_rng(77)
    centres = rng.random((40, 3)) * [10, 10, 2]
    sigma = 10.0 ** rng.uniform(-2.5, -0.5, 40)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 40, n)
    p = centres[k] + rng.normal(0, 1, (n, 3)) * sigma[k][:, None]
    p[:50] = rng.uniform(-500, 500, (50, 3))
    return p.astype(F)


LATTICE_V = F(0.0625) * F(1.1)


def lattice_cloud():
    """(i v, j v, 0) for i in -3..19 and j in 0..4, products in float32, with each point's float predecessor and
    successor on every coordinate: points exactly on voxel faces and one ulp to either side."""
    base = np.array([[F(i) * LATTICE_V, F(j) * LATTICE_V, F(0)] for i in range(-3, 20) for j in range(5)], F)
    return np.concatenate([base, np.nextafter(base, F(-np.inf)), np.nextafter(base, F(np.inf))]).astype(F)


def same_cloud():
    """1 000 copies of one point and one other point: two voxels."""
    return np.concatenate([np.tile(np.array([[0.3, 1000.7, -5.1]], F), (1000, 1)), np.array([[0.3, 1001.7, -5.1]], F)])


def _adv():
    Q, _, R = adversarial_cloud()
    return Q, F(R)


# name -> (points f32 [n, 3], voxel edge as a float32)
CASES = {
    "random": lambda: (random_cloud()[0], F(0.25)),
    "line_0.01": lambda: (line_cloud()[1], F(0.01)),
    "line_0.0025": lambda: (line_cloud()[1], F(0.0025)),
    "adversarial_R": lambda: _adv(),
    "adversarial_4R": lambda: (_adv()[0], F(4) * _adv()[1]),
    "clustered_0.02": lambda: (clustered(1, 100_000), F(0.02)),
    "clustered_0.1": lambda: (clustered(1, 100_000), F(0.1)),
    "lattice": lambda: (lattice_cloud(), LATTICE_V),
    "same": lambda: (same_cloud(), F(0.05)),
    "nonfinite": lambda: (nonfinite_cloud()[0].copy(), F(0.25)),
    "all_nan": lambda: (np.full((7, 3), np.nan, F), F(0.25)),
    "empty": lambda: (np.empty((0, 3), F), F(0.25)),
    "one": lambda: (np.array([[0.3, 1000.7, -5.1]], F), F(0.05)),
}


def reference(P, v, C=None):
    """The contract in numpy: (xyz f32 [k, 3], rgb u8 [k, 3] or None, first i32 [k], count i32 [k], mean64 f64 [k, 3]:
    the float64 mean of each voxel's points, for the error bound)."""
    P = np.ascontiguousarray(P, F).reshape(-1, 3)
    idx = np.nonzero(np.isfinite(P).all(axis=1))[0]
    if len(idx) == 0:
        return (np.empty((0, 3), F), None if C is None else np.empty((0, 3), np.uint8), np.empty(0, np.int32),
                np.empty(0, np.int32), np.empty((0, 3)))
    X = P[idx].astype(np.float64)
    o = X.min(axis=0)
    h = np.float64(F(v))
    u = (X - o) / h
    c = np.floor(u)
    assert u.max() < 2.0 ** 30
    f = u - c
    assert (f >= 0).all() and (f < 1).all()
    q = (f * 4294967296.0).astype(np.uint64)
    cells, inv = np.unique(c.astype(np.int64), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    k = len(cells)
    first = np.full(k, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, inv, idx)
    count = np.bincount(inv, minlength=k).astype(np.int64)
    S = np.zeros((k, 3), np.uint64)
    np.add.at(S, inv, q)
    mean64 = np.zeros((k, 3))
    np.add.at(mean64, inv, X)
    mean64 /= count[:, None]
    t = (S.astype(np.float64) / count[:, None].astype(np.float64)) * 2.0 ** -32
    xyz = (o + (cells.astype(np.float64) + t) * h).astype(F)
    rgb = None
    if C is not None:
        cs = np.zeros((k, 3), np.uint64)
        np.add.at(cs, inv, np.ascontiguousarray(C, np.uint8).reshape(-1, 3)[idx].astype(np.uint64))
        n2 = (2 * count[:, None]).astype(np.uint64)
        rgb = ((2 * cs + count[:, None].astype(np.uint64)) // n2).astype(np.uint8)
    order = np.argsort(first, kind="stable")
    return (xyz[order], None if rgb is None else rgb[order], first[order].astype(np.int32), count[order].astype(np.int32),
            mean64[order])


_cache = {}


def voxel_case(name):
    """(points, v, colours, reference without colours, reference with colours), computed once and read-only."""
    if name not in _cache:
        P, v = CASES[name]()
        C = np.random.default_rng(len(P) + 11).integers(0, 256, (len(P), 3)).astype(np.uint8)
        plain, col = reference(P, v), reference(P, v, C)
        for a in (P, C) + tuple(x for x in plain + col if x is not None):
            a.setflags(write=False)
        _cache[name] = (P, v, C, plain, col)
    return _cache[name]
