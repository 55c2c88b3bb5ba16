"""Inputs of the pass-path tests (test_pass_paths.py on the oracle, test_gpu_pass_paths.py on the device):
synthetic.make_scene scenes whose edge, low-resolution edge, label and weak maps are replaced by hand-built
ones, so that one pass takes the decisions that the scenes of make_scene at 24..160 px never take.

Which decisions those are is counted by the oracle (oracle.PATH_STATS, dpe_oracle.cpp ORACLE_PATH_STATS):
 * the strong sweep's edge scheme scans max(H, W) / 30 pixels at most towards an edge, so below 720 px every
   scan has 11 steps of 2 pixels; more than 16 steps (a third batch of 8 loads), steps longer than 2, the
   odd-length decrement of the four axis directions and an edge ray used beyond 64 pixels need ~2000 px;
 * labels of -1 and foreign labels, pixels with no STRONG pixel within 100, 64 full support slots, a
   (2r+1)^2 window of label 0 and low-resolution indices out of range need maps make_scene does not draw.
Every case is a valid input: sizes, maps and parameters the staging code accepts.  DESIGN.md §4, row "pass paths".
"""
import functools

import numpy as np

import oracle
from DPE_MVS import _abi, synthetic
from test_gpu_parity import _params

S, W_ = _abi.STRONG, _abi.WEAK


def _low(edge, low_scale=2):
    """The low-resolution edge map of a full one, as synthetic.make_scene builds it (any over 2 x 2)."""
    H, W = edge.shape
    lw, lh = (W + low_scale - 1) // low_scale, (H + low_scale - 1) // low_scale
    pad = np.zeros((lh * low_scale, lw * low_scale), bool)
    pad[:H, :W] = edge != 0
    return (pad.reshape(lh, low_scale, lw, low_scale).any(axis=(1, 3)) * 255).astype(np.uint8)


def _build(W, H, iters, *, edit=None, rotate_time=2, over=None):
    """(pass input, state, params) of a W x H, 3-view REFINE_ITER + geom pass.  `edit(scene, state)` replaces
    maps of the copied scene dict and of the ground-truth state in place."""
    base = synthetic.make_scene(W, H, 3)
    sc = dict(base, edge=base["edge"].copy(), edge_low=base["edge_low"].copy(), label=base["label"].copy())
    st = synthetic.gt_state(sc, seed=W + H)
    if edit is not None:
        edit(sc, st)
    p = _params("refine_iter", iters)
    p.rotate_time = rotate_time
    for k, v in (over or {}).items():
        setattr(p, k, v)
    inp = synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc), seed=W * 7 + 3)
    return inp, st, p


def _set_edges(sc, edge):
    sc["edge"] = (edge != 0).astype(np.uint8) * 255
    sc["edge_low"] = _low(sc["edge"])


# ---- the strong sweep's edge scheme ------------------------------------------------------------
def thin_2100x16():
    """max_edge_dist 70: step_num 22 almost everywhere, odd step lengths 3 -> 2 on the axis directions."""
    return _build(2100, 16, 2)


def thin_2880x14():
    """max_edge_dist 96: step_len 4 on the axis directions, 3 on the diagonals."""
    return _build(2880, 14, 2)


def wide_2100x96():
    """High enough for diagonal rays that find an edge 50..70 steps away: diagonal step_len 3, ray used."""
    return _build(2100, 96, 1)


def edge_lines_2880x96():
    """Hand-built edges on a 2880 x 96 image: vertical lines with gaps cycling through 40..260 px, so that
    the horizontal rays found cover every distance to 96 (step_num 11..22, step_len 2, 3 -> 2 and 4) and
    whole stretches are clipped; two-pixel-thick diagonals of both slopes through the wide gaps, for
    vertical rays and for diagonal rays that cross them; diagonal rays that reach a vertical line after
    88..95 steps give the diagonal step_len 4.  Rays of 64 steps and more are used (k_edge_rays carries
    its nearest edge across more than one 64-lane step)."""
    def edit(sc, st):
        H, W = sc["edge"].shape
        e = np.zeros((H, W), bool)
        gaps, x, k, xs = [40, 58, 77, 96, 131, 170, 199, 260], 23, 0, []
        while x < W - 8:
            e[:, x] = True
            xs.append(x)
            x += gaps[k % len(gaps)]
            k += 1
        ys = np.arange(H)
        for j in range(len(xs) - 1):
            a, b = xs[j], xs[j + 1]
            if b - a == 170:      # a diagonal of each slope inside the gap, 2 px thick
                for s in (0, 1):
                    e[ys, np.clip(a + 30 + ys + s, 0, W - 1)] = True
            if b - a == 260:
                for s in (0, 1):
                    e[ys, np.clip(b - 40 - ys - s, 0, W - 1)] = True
        _set_edges(sc, e)
    return _build(2880, 96, 1, edit=edit)


def tall_40x150():
    """Column scans with carries: edges on rows 0, 63, 64, 127, 128 and 149 (k_edge_rays steps 64 rows at
    a time), STRONG pixels only in rows 0 and 149 of every third column (k_strong_tables_scan carries a
    row index over two steps; the rings of k_find_nearest_strong grow to 74)."""
    def edit(sc, st):
        H, W = sc["edge"].shape
        e = np.zeros((H, W), bool)
        e[[0, 63, 64, 127, 128, 149], :] = True
        _set_edges(sc, e)
        st["weak"][:] = W_
        st["weak"][0, 2::3] = S
        st["weak"][149, 1::3] = S
    return _build(40, 150, 1, edit=edit)


# ---- the set-up chain --------------------------------------------------------------------------
def one_column_230x40():
    """Every pixel WEAK but column x = 8: the nearest STRONG pixel lies |x - 8| away, at r == 100 for
    x = 108 and nowhere for x >= 109; probes read "none", low-resolution walk indices leave the map at the
    last row, most pixels keep <= 3 support points."""
    def edit(sc, st):
        st["weak"][:] = W_
        st["weak"][:, 8] = S
    return _build(230, 40, 1, edit=edit)


def all_weak_48x32():
    """No STRONG pixel at all: every probe reads none, every pixel has no support point, NeigbourUpdate
    turns every pixel UNKNOWN."""
    def edit(sc, st):
        st["weak"][:] = W_
    return _build(48, 32, 1, edit=edit)


def _lattice_labels(sc, st):
    H, W = sc["label"].shape
    lab = np.ones((H, W), np.int32)
    lab[::9, :] = 2                      # foreign rows
    lab[:, ::17] = -1                    # columns that stop a label ray
    lab[4::11, 5::13] = 0                # dots of "no label"
    sc["label"] = lab
    st["weak"][:] = S
    st["weak"][6:-6:2, 6:-6:3] = W_


def lattice_96x64():
    """Labels 1 with -1 columns every 17, label-2 rows every 9 and label-0 dots; a WEAK lattice in a STRONG
    image: label rays stop on -1, run on past foreign labels, extension points are dropped for a foreign
    label."""
    return _build(96, 64, 1, edit=_lattice_labels)


def full_slots_128x96():
    """rotate_time 4, one label, no edges, a sparse WEAK lattice in a STRONG image: every probe and every
    extension step finds a point, so the support sets reach all 64 slots."""
    def edit(sc, st):
        sc["label"] = np.ones_like(sc["label"])
        _set_edges(sc, np.zeros(sc["edge"].shape, bool))
        st["weak"][:] = S
        st["weak"][8:-8:8, 8:-8:8] = W_
    return _build(128, 96, 1, edit=edit, rotate_time=4)


def _label0_block(radius, increment):
    """A 23 x 23 block of label 0 (a segmentation hole) with WEAK pixels in and around it: windows of
    (2r+1)^2 pixels that are all label 0 make bound_pix / tot_pix 1 and the edge limit random-off."""
    def edit(sc, st):
        lab = sc["label"]
        lab[18:41, 28:51] = 0
        st["weak"][12:47, 22:57] = W_
    return _build(80, 60, 1, edit=edit, over=dict(strong_radius=radius, strong_increment=increment))


def label0_block_r5():
    return _label0_block(5, 2)


def label0_block_r8():
    """strong_radius 8: the largest window k_gen_edge_inform counts from its LDS tile."""
    return _label0_block(8, 4)


def label0_block_r9():
    """strong_radius 9: k_gen_edge_inform's untiled window loop."""
    return _label0_block(9, 3)


CASES = {f.__name__: f for f in (
    thin_2100x16, thin_2880x14, wide_2100x96, edge_lines_2880x96, tall_40x150, one_column_230x40, all_weak_48x32,
    lattice_96x64, full_slots_128x96, label0_block_r5, label0_block_r8, label0_block_r9)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(pass input, state, params) of a named case.  Shared; callers do not modify."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """(outputs, decision-path counts) of the oracle's pass over case(name).  Shared; callers do not modify."""
    inp, st, _ = case(name)
    out = oracle.run_pass(inp, st)
    return out, oracle.last_path_stats()


# The suite's older pass inputs, for the census of what they reach (test_pass_paths.py)
def older_input(W, H, N, kind, iters=3):
    sc = synthetic.make_scene(W, H, N)
    p = _params(kind, iters)
    st = synthetic.first_init_state(sc) if kind == "first" else synthetic.gt_state(sc, seed=W + H)
    inp = synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc) if p.geom_consistency else None, seed=W * 7 + N)
    return inp, st


OLDER = {"iter_80x60": (80, 60, 4, "refine_iter"), "init_80x60": (80, 60, 4, "refine_init"),
         "acmh_57x43": (57, 43, 3, "acmh_geom"), "first_64x48": (64, 48, 3, "first")}


@functools.lru_cache(maxsize=None)
def oracle_older(name):
    inp, st = older_input(*OLDER[name])
    out = oracle.run_pass(inp, st)
    return out, oracle.last_path_stats()
