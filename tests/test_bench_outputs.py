"""bench.py's plain run and --dump-outputs: the plain line carries the headline fields and none of
the side measurements (those need --full), --steps sets the number of timed steps, and the dumped
arrays are what the pass leaves for a caller (dpe_pm_fetch), within the 64 MB budget."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline", "gather_roof", "kernel_ms", "work", "pass_types_mpix_s", "pass_levels", "pipeline_config4",
             "pipeline_config5", "end_to_end", "cpu_baseline", "parity")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _state(h, w, seed=3):
    rng = np.random.default_rng(seed)
    return {"planes": rng.standard_normal((h, w, 4)).astype(np.float32),
            "weak": rng.integers(0, 4, (h, w)).astype(np.uint8),
            "sel": rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32),
            "costs": rng.random((h, w)).astype(np.float32)}


FILES = ["costs.npy", "costs_nonfinite.npy", "planes.npy", "sel.npy", "weak.npy"]


def _restore(folder, k, dtype):
    """What the pass stored, from the dumped pair: the finite values, NaN / inf put back by their code."""
    a = np.load(os.path.join(folder, f"{k}.npy"))
    assert np.isfinite(a).all(), k
    p = os.path.join(folder, f"{k}_nonfinite.npy")
    if os.path.exists(p):
        code = np.load(p)
        assert code.dtype == np.float32 and code.shape == a.shape and (a[code != 0] == 0).all()
        for c, v in ((1, np.nan), (2, np.inf), (3, -np.inf)):
            a = np.where(code == c, np.float32(v), a)
    return a.astype(dtype)


def test_dump_outputs_whole_frame(tmp_path):
    bench = _bench_module()
    st = _state(30, 41)
    info = bench.dump_outputs(str(tmp_path / "o"), st)
    assert not info["sampled"] and sorted(k + ".npy" for k in info["arrays"]) == FILES
    assert not np.load(tmp_path / "o" / "costs_nonfinite.npy").any()
    for k, v in st.items():
        a = np.load(tmp_path / "o" / f"{k}.npy")
        assert a.dtype == (np.float64 if k == "sel" else np.float32)
        assert a.shape == v.shape and np.array_equal(a, v.astype(a.dtype))
        assert np.array_equal(a.astype(v.dtype), v)          # the stored format loses nothing


def test_dump_outputs_are_finite_and_lose_nothing(tmp_path):
    """NaN / inf values of the pass are written as 0 with their kind in <name>_nonfinite.npy; view
    masks of up to 24 source views fit float32 exactly."""
    bench = _bench_module()
    st = _state(19, 23)
    st["sel"] &= np.uint32(2 ** 24 - 1)
    st["costs"][3, 5] = np.nan
    st["costs"][4, 0] = np.inf
    st["costs"][18, 22] = -np.inf
    st["planes"][7, 7, 2] = np.nan
    info = bench.dump_outputs(str(tmp_path / "o"), st, num_images=25)
    assert sorted(k + ".npy" for k in info["arrays"]) == sorted(FILES + ["planes_nonfinite.npy"])
    assert np.load(tmp_path / "o" / "sel.npy").dtype == np.float32
    for k, v in st.items():
        assert np.array_equal(_restore(tmp_path / "o", k, v.dtype).view(np.uint8), v.view(np.uint8)), k


def test_dump_outputs_samples_a_frame_over_the_budget(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20000)
    st = _state(37, 53)
    a = bench.dump_outputs(str(tmp_path / "a"), st)
    b = bench.dump_outputs(str(tmp_path / "b"), st)
    assert a["sampled"] and a["bytes"] <= 20000
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(FILES + ["pixels.npy"])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 20000 + 128 * len(files)
    pix = np.load(tmp_path / "a" / "pixels.npy").astype(np.int64)
    assert np.all(np.diff(pix) > 0) and pix[0] >= 0 and pix[-1] < 37 * 53
    for f in files:                                          # the same sample on every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    assert np.array_equal(np.load(tmp_path / "a" / "planes.npy"), st["planes"].reshape(-1, 4)[pix])
    assert np.array_equal(np.load(tmp_path / "a" / "sel.npy"), st["sel"].reshape(-1)[pix].astype(np.float64))


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--launch-check"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--steps 0" in r.stderr


@pytest.mark.gpu
def test_gpu_plain_run_line_and_dumped_outputs(tmp_path):
    """One plain run at a small frame: the line has the headline fields and nothing that needs --full;
    the dumped arrays equal a fresh pass on the same inputs through DPE_MVS.native (the pass restarts
    from the staged state at every execute, so the last of 3 timed steps equals a single one)."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--width", "200",
                        "--height", "152", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    (line,) = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert line["unit"] == "Mpix/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(200 * 152 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(out)) == FILES

    bench = _bench_module()
    from DPE_MVS import _abi, native, synthetic
    sc = synthetic.make_scene(200, 152, bench.NV_, seed=synthetic.SCENE_SEED)
    inp = synthetic.pass_input(sc, bench.workload_params(_abi, bench.NV_), depths=synthetic.src_depths(sc))
    ref = native.run_pass(inp, synthetic.gt_state(sc), device=0)
    for k, v in ref.items():
        a = np.load(out / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == v.shape and np.isfinite(a).all()
        back = _restore(out, k, v.dtype)
        if k == "costs":    # bit for bit where finite; a NaN stays a NaN (its payload is not kept)
            assert np.array_equal(np.isnan(back), np.isnan(v))
            back, v = np.nan_to_num(back, nan=0.0), np.nan_to_num(v, nan=0.0)
        assert np.array_equal(back.view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k
