"""The viz medium results (RunDPEPipeline's `viz` flag, main.cpp:361-364, 380-383, 448-454): the
baseline JPEG encoder that stands in for cv::imwrite (host/jpeg_enc.cpp), the ShowDepthMap /
ShowNormalMap / ShowWeakImage renderers (host/viz.cpp, DPE.cpp:384-502) and the pipeline wiring.

The encoder's yardstick is libjpeg through PIL: our file must decode, pixel for pixel, to what
libjpeg's own encoding of the same pixels (quality 95, 4:2:0, baseline, default Huffman tables)
decodes to.  A baseline decode is a function of the quantised coefficients alone, so this equality
pins the colour conversion, chroma averaging, edge padding, forward DCT and quantisation to
libjpeg's arithmetic without a tolerance.  (Against libjpeg-turbo 3 the files are in fact
byte-identical; the tests do not ask for that.)"""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from DPE_MVS import _abi, pipeline, synthetic
from test_pipeline import oracle_runner, _copy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOUR_SHAPES = [(9, 17), (33, 50), (48, 64), (37, 259)]
GREY_SHAPES = [(30, 40), (9, 17)]


def noisy_gradient_bgr(h, w):
    """The colour image of tests/test_fusion.py:47-51, read as BGR."""
    rng = np.random.default_rng(h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 7) % 256], -1)
    return np.clip(img + rng.integers(-30, 30, img.shape), 0, 255).astype(np.uint8)


def edge_like_grey(h, w):
    """A 0 / 255 map with thin lines, like EdgeSegment's edges."""
    g = np.zeros((h, w), np.uint8)
    g[::7, :] = 255
    g[:, 3::11] = 255
    yy, xx = np.mgrid[0:h, 0:w]
    g[(yy + xx) % 13 == 0] = 255
    return g


def _pil_jpeg(img):
    """libjpeg's encoding of a BGR or grey image with cv::imwrite's settings."""
    bio = io.BytesIO()
    if img.ndim == 3:
        Image.fromarray(np.ascontiguousarray(img[..., ::-1]), mode="RGB").save(bio, format="JPEG", quality=95, subsampling=2)
    else:
        Image.fromarray(img, mode="L").save(bio, format="JPEG", quality=95)
    return bio.getvalue()


# ------------------------------------------------------------------------------ 1. encoder against libjpeg
@pytest.mark.parametrize("shape,colour", [(s, True) for s in COLOUR_SHAPES] + [(s, False) for s in GREY_SHAPES])
def test_encoder_matches_libjpeg(tmp_path, shape, colour):
    img = noisy_gradient_bgr(*shape) if colour else edge_like_grey(*shape)
    p = str(tmp_path / "ours.jpg")
    pipeline.write_jpeg(p, img, quality=95)
    ours = Image.open(p)
    ref = Image.open(io.BytesIO(_pil_jpeg(img)))
    assert ours.size == (shape[1], shape[0])
    if colour:
        assert ours.mode == "RGB" and ours.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    else:
        assert ours.mode == "L" and len(ours.layer) == 1 and ours.layer[0][1:3] == (1, 1)
    assert {k: list(v) for k, v in ours.quantization.items()} == {k: list(v) for k, v in ref.quantization.items()}
    assert not ours.info.get("progressive") and not ours.info.get("progression")
    assert ours.info.get("jfif") is not None                      # the JFIF APP0 segment
    a, b = np.asarray(ours), np.asarray(ref)
    assert a.shape == b.shape and np.array_equal(a, b)            # the pin to libjpeg's encoder
    if colour:
        assert np.array_equal(pipeline.read_bgr(p), a[..., ::-1])
    else:
        assert np.array_equal(pipeline.read_gray(p), a)
        assert np.array_equal(pipeline.read_bgr(p), np.repeat(a[..., None], 3, -1))


def test_encoder_split_halves_chain(tmp_path):
    """write_jpeg is jpeg_blocks followed by the back half; the size query counts MCU blocks."""
    img = noisy_gradient_bgr(33, 50)
    blocks = pipeline.jpeg_blocks(img)
    assert blocks.shape == (3 * 4 * 6, 64) and blocks.dtype == np.int16
    pipeline.write_jpeg_blocks(str(tmp_path / "b.jpg"), blocks, 50, 33)
    pipeline.write_jpeg(str(tmp_path / "a.jpg"), img)
    assert open(tmp_path / "a.jpg", "rb").read() == open(tmp_path / "b.jpg", "rb").read()
    assert pipeline.jpeg_blocks(edge_like_grey(9, 17)).shape == (2 * 3, 64)
    # natural (row-major) coefficient order: a horizontal ramp has energy in the first row only
    ramp = np.repeat(np.tile((np.arange(8) * 30).astype(np.uint8), (8, 1))[..., None], 3, -1)
    b = pipeline.jpeg_blocks(np.ascontiguousarray(ramp))[0].reshape(8, 8)
    assert b[0, 1] != 0 and not b[1:, :].any()


# ------------------------------------------------------------------------------ 2. renderer KATs
F = np.float32


def _pixel_val(d, dmin, dmax):
    v = F(F(dmax - d) / F(dmax - dmin))
    v = min(max(v, F(0)), F(1))
    return min(max(F(v * F(255)), F(0)), F(255))


def ref_depth_px(d, dmin, dmax):
    """ShowDepthMap (DPE.cpp:391-442) in numpy float32 / float64, BGR."""
    d, dmin, dmax = F(d), F(dmin), F(dmax)
    if d < dmin or d > dmax or np.isnan(d):
        return (0, 0, 0)
    v = _pixel_val(d, dmin, dmax)
    if v <= 51:
        return (255, int(F(v * F(5))), 0)
    if v <= 102:
        v = F(v - F(51))
        return (int(F(F(255) - F(v * F(5)))), 255, 0)
    if v <= 153:
        v = F(v - F(102))
        return (0, 255, int(F(v * F(5))))
    if v <= 204:
        v = F(v - F(153))
        return (0, 255 - int(np.float64(v) * 128.0 / 51 + 0.5), 255)
    v = F(v - F(204))
    return (0, 127 - int(np.float64(v) * 127.0 / 51 + 0.5), 255)


def depth_hitting(target, dmin, dmax):
    """A depth whose pixel_val is exactly `target` (searched among the floats around the solution)."""
    d = F(dmax - F(target) / F(255) * F(dmax - dmin))
    cands = [d]
    lo = hi = d
    for _ in range(8):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        cands += [lo, hi]
    for c in cands:
        if dmin <= c <= dmax and _pixel_val(c, dmin, dmax) == F(target):
            return c
    raise AssertionError(f"no float32 depth gives pixel_val {target}")


def depth_kat_inputs():
    dmin, dmax = F(1.5), F(4.0)
    on = [depth_hitting(t, dmin, dmax) for t in (51, 102, 153, 204, 255)]
    inside = [F(dmax - F(t) / F(255) * F(dmax - dmin)) for t in (20.3, 77.7, 130.2, 180.6, 230.9)]
    inside += [F(3.1234), F(2.71), F(1.9), F(1.6), F(3.9)]
    d = np.array([F(1.25), F(4.5), F(np.nan), dmin, dmax, F(0.0), F(-1.0), F(np.inf)] + on + inside, np.float32)
    return d, dmin, dmax


def test_depth_render_kat():
    d, dmin, dmax = depth_kat_inputs()
    got = pipeline.viz_render(pipeline.VIZ_DEPTH, depth=d.reshape(1, -1), dmin=dmin, dmax=dmax)[0]
    want = np.array([ref_depth_px(x, dmin, dmax) for x in d], np.uint8)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    # the literal corners of the ramp: below / above / NaN black, max depth blue, the segment ends
    assert got[:5].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 255], [255, 0, 0]]
    assert got[8:13].tolist() == [[255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 127, 255], [0, 0, 255]]
    segs = [0 if v <= 51 else 1 if v <= 102 else 2 if v <= 153 else 3 if v <= 204 else 4
            for v in (_pixel_val(x, dmin, dmax) for x in d[13:18])]
    assert segs == [0, 1, 2, 3, 4]                                 # one depth inside each segment


def ref_normal_px(n):
    x, y, z = (np.float64(F(c)) for c in n)
    with np.errstate(all="ignore"):
        norm = F(np.sqrt(x * x + y * y + z * z))
        v = np.zeros(3, np.float32) if norm == 0 else np.array([F(F(c) * F(F(1) / norm)) for c in n], np.float32)
        t = np.rint(v * F(127.5) + F(127.5))                      # float32, unfused; rint = half to even
    return tuple(0 if np.isnan(q) else int(min(max(q, 0), 255)) for q in t)


def normal_kat_inputs():
    return np.array([[0, 0, 0], [np.nan, 0.5, 0.5], [0.3, np.nan, -0.2], [1, 2, 2], [2, 4, 4], [-1, -2, -2], [0, 0, 1],
                     [0, -3, 0], [3, 4, 0], [-8, 15, 0], [1e-20, 0, 0], [0.123, -0.456, 0.789], [1e30, 1e30, 1e30],
                     [np.inf, 1, 1]], np.float32)


def test_normal_render_kat():
    n = normal_kat_inputs()
    got = pipeline.viz_render(pipeline.VIZ_NORMAL, normal=n.reshape(1, -1, 3))[0]
    want = np.array([ref_normal_px(v) for v in n], np.uint8)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert got[0].tolist() == [128, 128, 128]                      # zero vector: 127.5 ties to the even 128
    assert got[1].tolist() == [0, 0, 0] and got[2].tolist() == [0, 0, 0]   # NaN anywhere -> NaN length -> 0
    # (1, 2, 2) / 3: 2/3 * 127.5 + 127.5 is exactly 212.5 in float32 -> 212 (half to even, not 213)
    assert got[3].tolist() == [170, 212, 212] and got[4].tolist() == [170, 212, 212]
    assert got[6].tolist() == [128, 128, 255] and got[7].tolist() == [128, 0, 128]


def test_weak_render_kat():
    w = np.array([[0, 1, 2, 3, 200]], np.uint8)
    got = pipeline.viz_render(pipeline.VIZ_WEAK, weak=w)[0]
    assert (_abi.WEAK, _abi.STRONG, _abi.UNKNOWN) == (0, 1, 2)
    assert got.tolist() == [[255, 255, 255], [0, 255, 0], [0, 0, 255], [0, 0, 0], [0, 0, 0]]


# ------------------------------------------------------------------------------ 3. pipeline
def level_sizes(W, H):
    """(w, h) of pass 0..7 of a two-round schedule."""
    half = (pipeline.std_round(W * 0.5), pipeline.std_round(H * 0.5))
    return [half] * 4 + [(W, H)] * 4


def remove_maps_of_image0(folder):
    """Image 0's edges_<s>.dmb / labels_<s>.dmb: GetProblemEdges then computes them (scales 0 and 1)."""
    rf = os.path.join(folder, "DPE", "00000000")
    for f in os.listdir(rf):
        if f.startswith(("edges_", "labels_")):
            os.remove(os.path.join(rf, f))


def jpgs_under(folder):
    return sorted(os.path.relpath(os.path.join(r, f), folder) for r, _, fs in os.walk(os.path.join(folder, "DPE"))
                  for f in fs if f.endswith(".jpg"))


def weak_colouring(weak_npy):
    """ShowWeakImage of weak.npy's encoding (1 = WEAK, 2 = STRONG, 0 = UNKNOWN), BGR."""
    out = np.zeros(weak_npy.shape + (3,), np.uint8)
    out[weak_npy == 1] = (255, 255, 255)
    out[weak_npy == 2] = (0, 255, 0)
    out[weak_npy == 0] = (0, 0, 255)
    return out


def check_viz_folder(folder, W=64, H=48, n=4):
    sizes = level_sizes(W, H)
    want = []
    for i in range(n):
        rf = os.path.join(folder, "DPE", f"{i:08d}")
        for it in range(8):
            for name in ("depth", "normal", "weak"):
                p = os.path.join(rf, f"{name}_{it}.jpg")
                assert os.path.exists(p), p
                im = Image.open(p)
                assert im.size == sizes[it] and im.mode == "RGB", (p, im.size)
                assert pipeline.read_bgr(p).shape == (sizes[it][1], sizes[it][0], 3)
                want.append(os.path.relpath(p, folder))
    rf0 = os.path.join(folder, "DPE", "00000000")
    for s, (w, h) in ((0, (W, H)), (1, sizes[0])):                 # the scales computed for image 0
        e = Image.open(os.path.join(rf0, f"rawedge_{s}.jpg"))
        assert e.mode == "L" and e.size == (w, h)
        c = Image.open(os.path.join(rf0, f"connect_{s}.jpg"))
        assert c.mode == "RGB" and c.size == (w, h)
        want += [os.path.join("DPE", "00000000", f"rawedge_{s}.jpg"), os.path.join("DPE", "00000000", f"connect_{s}.jpg")]
    assert jpgs_under(folder) == sorted(want)                      # and no picture beside a map that was read
    return want


@pytest.fixture(scope="module")
def viz_runs(tmp_path_factory):
    """The 64x48x4 folder run with the oracle runner, once with viz and once without."""
    base = tmp_path_factory.mktemp("vizdense")
    src = str(base / "src")
    synthetic.write_dense_folder(src, 64, 48, 4)
    remove_maps_of_image0(src)
    on, off = _copy(src, base, "on"), _copy(src, base, "off")
    assert pipeline.run_dpe_pipeline(on, runner=oracle_runner(), normal=True, weak=True, verbose=False, viz=True,
                                     keep_intermediate=True) == 0
    assert pipeline.run_dpe_pipeline(off, runner=oracle_runner(), normal=True, weak=True, verbose=False, viz=False,
                                     keep_intermediate=True) == 0
    return src, on, off


def test_pipeline_writes_the_viz_pictures(viz_runs):
    """Fails without the feature: `viz` was accepted and dropped."""
    _, on, _ = viz_runs
    check_viz_folder(on)
    for i in range(4):
        rf = os.path.join(on, "DPE", f"{i:08d}")
        weak = np.load(os.path.join(rf, "weak.npy"))
        colour = weak_colouring(weak)
        p = os.path.join(rf, "weak_7.jpg")
        # libjpeg's own encoding of the colouring decodes to exactly our file's pixels ...
        assert np.array_equal(np.asarray(Image.open(p)), np.asarray(Image.open(io.BytesIO(_pil_jpeg(colour)))))
        # ... and the luma plane is the colouring's within the quantisation error: every one of the 64
        # coefficients is off by at most q/2 and weighs at most 1/4 in a pixel, plus 1 for the
        # decoder's rounding
        im = Image.open(p)
        im.draft("YCbCr", im.size)
        y = np.asarray(im)[..., 0].astype(int)
        b, g, r = (colour[..., k].astype(int) for k in range(3))
        y_true = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
        bound = sum(Image.open(p).quantization[0]) / 8 + 1
        assert np.abs(y - y_true).max() <= bound, (np.abs(y - y_true).max(), bound)
    # rawedge is the edge map that was written
    rf0 = os.path.join(on, "DPE", "00000000")
    for s in (0, 1):
        e = pipeline.read_bin_mat(os.path.join(rf0, f"edges_{s}.dmb"))
        raw = np.asarray(Image.open(os.path.join(rf0, f"rawedge_{s}.jpg")))
        assert np.array_equal(raw, np.asarray(Image.open(io.BytesIO(_pil_jpeg(e)))))


def colour_of_labels(lab):
    out = np.zeros(lab.shape + (3,), np.uint8)
    for v in np.unique(lab):
        out[lab == v] = pipeline.connect_color(int(v))
    return out


def test_connect_picture_is_taken_before_small_regions_go(viz_runs):
    """connect_<s>.jpg: colors[label] of every pixel before the small regions become -1, from the same
    segmentation as the labels; label 0 black, the colour a fixed hash of the label (the reference's
    unseeded rand() is not reproducible)."""
    img = np.full((128, 192), 90, np.uint8)                       # flat ground, bright cell walls ...
    img[::32, :] = 250
    img[:, ::48] = 250
    img[40:60, 40:60] = 250                                       # ... and a walled cell too small to keep
    img[44:56, 44:56] = 90
    lab, con = pipeline.edge_segment_connect(0, img)
    assert np.array_equal(lab, pipeline.edge_segment(0, img, 1, False, True))      # modes 0 / 1 unchanged
    assert (lab == -1).any() and (lab > 0).any() and (lab == 0).any()
    keep = lab >= 0
    assert np.array_equal(con[keep], colour_of_labels(lab)[keep])
    small = con[lab == -1]                                        # label 9 is the one missing from the map
    assert sorted(set(np.unique(lab)) - {-1, 0}) == [k for k in range(1, 18) if k != 9]
    assert (small == np.array(pipeline.connect_color(9), np.uint8)).all()   # it still carries its colour
    assert len({pipeline.connect_color(k) for k in range(1, 200)}) == 199
    # in the pipeline: the picture of the labels that were written (the synthetic scene has no small region)
    _, on, _ = viz_runs
    rf0 = os.path.join(on, "DPE", "00000000")
    for s in (0, 1):
        lab = pipeline.read_bin_mat(os.path.join(rf0, f"labels_{s}.dmb"))
        assert (lab >= 0).all()
        got = np.asarray(Image.open(os.path.join(rf0, f"connect_{s}.jpg")))
        assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(_pil_jpeg(colour_of_labels(lab))))))


def test_viz_off_writes_no_picture_and_changes_no_output(viz_runs):
    _, on, off = viz_runs
    assert jpgs_under(off) == []
    for i in range(4):
        for f in ("depth.npy", "normal.npy", "weak.npy"):
            a = open(os.path.join(on, "DPE", f"{i:08d}", f), "rb").read()
            b = open(os.path.join(off, "DPE", f"{i:08d}", f), "rb").read()
            assert a == b, (i, f)
    for s in (0, 1):                                              # the computed maps too
        for f in (f"edges_{s}.dmb", f"labels_{s}.dmb"):
            a = open(os.path.join(on, "DPE", "00000000", f), "rb").read()
            assert a == open(os.path.join(off, "DPE", "00000000", f), "rb").read(), f


# ------------------------------------------------------------------------------ 4. ASan + UBSan
@pytest.mark.timeout(600)
def test_encoder_and_renderers_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/sanitize/viz_sanitize.cpp) encodes and renders at 1x1, 7x3, 17x9
    and 16x16 into exactly sized heap buffers; any report aborts it."""
    r = subprocess.run(["make", "-s", "sanitize-viz"], cwd=os.path.join(ROOT, "dpe-mvs_amd"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "dpe-mvs_amd", "bin", "viz_sanitize"), str(tmp_path)], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "viz sanitize ok" in r.stdout, r.stdout + r.stderr[-2000:]
    for w, h in ((1, 1), (7, 3), (17, 9), (16, 16)):              # what it wrote is a JPEG of that size
        assert Image.open(tmp_path / f"viz_{w}x{h}_3_0.jpg").size == (w, h)
        assert Image.open(tmp_path / f"viz_{w}x{h}_1_0.jpg").mode == "L"
