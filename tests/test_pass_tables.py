"""The pass-constant tables of dpe-mvs_amd/csrc/pass_tables.h (PassConst::spat36 and ::base_len).

The header is plain C++: it is compiled here with g++ (-ffp-contract=off, as the library is built)
and compared bit for bit with a float32 numpy restatement of the per-pixel expressions it replaces
(bilateral_weight's spatial term, baseline_and_weights' summand).  Every operation is a single
correctly rounded float32 operation in both, so the bits must agree.  That the kernels computed
those same bits per pixel is what the GPU parity suite checks against the oracle, which keeps the
per-pixel form."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "dpe-mvs_amd", "csrc", "pass_tables.h")
F = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_tables")
    src = d / "t.cpp"
    src.write_text(f'#include "{HDR}"\n'
                   'extern "C" void spat36(float ss, float* out) { dpe::build_spat36(ss, out); }\n'
                   'extern "C" float base_len(const float* c0, const float* cs) { return dpe::baseline_length(c0, cs); }\n')
    so = d / "t.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    lib.spat36.argtypes = [C.c_float, C.POINTER(C.c_float)]
    lib.base_len.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.base_len.restype = C.c_float
    return lib


@pytest.mark.parametrize("sigma", [5.0, 4.0, 0.7])
def test_spat36(lib, sigma):
    out = (C.c_float * 36)()
    lib.spat36(sigma, out)
    got = np.array(out, dtype=F)
    ss = F(sigma)
    want = np.empty(36, F)
    for k in range(36):
        xd, yd = F(-5 + 2 * (k // 6)), F(-5 + 2 * (k % 6))
        sd = np.sqrt(F(F(xd * xd) + F(yd * yd)))
        want[k] = F(-sd) / F(F(F(2.0) * ss) * ss)
    assert want.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got < 0) and got[0] == got[35] == got[5] == got[30]   # the four corners


def test_base_len(lib):
    rng = np.random.default_rng(3)
    for i in range(2000):
        scale = F(10.0 ** rng.uniform(-3, 3))
        c0 = (rng.normal(0, 1, 3) * scale).astype(F)
        cs = (c0 + rng.normal(0, 1, 3).astype(F) * F(10.0 ** rng.uniform(-4, 1)) * scale).astype(F)
        got = F(lib.base_len(c0.ctypes.data_as(C.POINTER(C.c_float)), cs.ctypes.data_as(C.POINTER(C.c_float))))
        d = c0 - cs
        assert d.dtype == F
        tv = F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))
        want = np.sqrt(tv)
        assert want.dtype == F and got.view(np.uint32) == want.view(np.uint32), (i, c0, cs, got, want)
