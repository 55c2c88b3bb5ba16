"""The lane map of the strong sweep's split pool tails (dpe-mvs_amd/csrc/pool_tail.h), compiled with
g++ and checked for every last-round size 1..64.  Both pools (cost vectors, refinement) call the one
map, so every check runs once per pool name over the same function.

  * each (job, row) of the round is covered by exactly one lane;
  * a job's lanes are adjacent, its rows ascending and contiguous from 0 to 5, and exactly its last
    lane is marked `last`;
  * the LDS slots a round uses are distinct and inside the 288-float tail region of the carve;
  * chaining the partial sums as the kernel does (first lane from zero, each later lane adds its
    rows in order to the partial it is handed) gives the serial row-order sum bit for bit.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "dpe-mvs_amd", "csrc", "pool_tail.h")
F = np.float32
POOLS = ["cost vectors", "refinement"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pool_tail")
    src = d / "t.cpp"
    src.write_text(f'#include "{HDR}"\n'
                   'extern "C" void lane_map(int tail, int lane, int* out) {\n'
                   '  const dpe::TailLane t = dpe::tail_lane(tail, lane);\n'
                   '  out[0] = t.job; out[1] = t.row0; out[2] = t.rows; out[3] = t.last;\n'
                   '}\n'
                   'extern "C" int lanes_per_job(int tail) { return dpe::tail_lanes_per_job(tail); }\n'
                   'extern "C" int lds_slot(int tail, int job, int a) { return dpe::tail_lds_slot(tail, job, a); }\n'
                   'extern "C" int max_jobs() { return dpe::kTailMaxJobs; }\n'
                   'extern "C" int lds_jobs() { return dpe::kTailLdsJobs; }\n')
    so = d / "t.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)], check=True)
    return C.CDLL(str(so))


def _map(lib, tail):
    out = (C.c_int * 4)()
    lanes = []
    for lane in range(64):
        lib.lane_map(tail, lane, out)
        lanes.append(tuple(out))
    return lanes


@pytest.mark.parametrize("pool", POOLS)
def test_every_row_covered_once(lib, pool):
    assert lib.max_jobs() == 32 and lib.lds_jobs() == 16
    for tail in range(1, 65):
        npc = lib.lanes_per_job(tail)
        assert npc == (6 if tail <= 10 else 3 if tail <= 16 else 2 if tail <= 32 else 1), tail
        assert tail * npc <= 64
        cover = np.zeros((tail, 6), int)
        per_job = {}
        for lane, (job, row0, rows, last) in enumerate(_map(lib, tail)):
            if job < 0:
                assert rows == 0 and lane >= tail * npc
                continue
            assert 0 <= job < tail and rows == 6 // npc and 0 <= row0 and row0 + rows <= 6
            cover[job, row0:row0 + rows] += 1
            per_job.setdefault(job, []).append((lane, row0, rows, last))
        assert np.all(cover == 1), (pool, tail)
        for job, ls in per_job.items():
            assert [l for l, *_ in ls] == list(range(ls[0][0], ls[0][0] + npc)), (tail, job)   # adjacent lanes
            nxt = 0
            for i, (lane, row0, rows, last) in enumerate(ls):
                assert row0 == nxt and bool(last) == (i == len(ls) - 1), (tail, job, lane)
                nxt = row0 + rows
            assert nxt == 6


@pytest.mark.parametrize("pool", POOLS)
def test_lds_slots_fit_the_tail_region(lib, pool):
    for tail in range(1, lib.max_jobs() + 1):
        npc = lib.lanes_per_job(tail)
        rows = range(3, 6) if npc == 2 else range(6)          # two lanes per job: rows 0..2 stay in registers
        slots = [lib.lds_slot(tail, job, a) for job in range(tail) for a in rows]
        used = sorted(s + k for s in slots for k in range(3))
        assert len(set(used)) == len(used) and used[0] >= 0 and used[-1] < lib.lds_jobs() * 18, (pool, tail)


@pytest.mark.parametrize("pool", POOLS)
def test_chained_partials_equal_the_serial_sum(lib, pool):
    rng = np.random.default_rng(11 + POOLS.index(pool))
    for tail in range(1, 65):
        # row triplets with mixed signs and magnitudes, so that a different association would show
        rows = (rng.normal(0, 1, (tail, 6, 3)) * 10.0 ** rng.uniform(-3, 3, (tail, 6, 1))).astype(F)
        serial = np.zeros((tail, 3), F)
        for a in range(6):
            serial = serial + rows[:, a]
        assert serial.dtype == F
        got = np.full((tail, 3), np.nan, F)
        handed = np.zeros(3, F)                                 # the partial of the lane below
        for lane, (job, row0, nrows, last) in enumerate(_map(lib, tail)):
            if job < 0:
                continue
            acc = np.zeros(3, F) if row0 == 0 else handed
            for a in range(row0, row0 + nrows):
                acc = acc + rows[job, a]
            assert acc.dtype == F
            handed = acc
            if last:
                got[job] = acc
        assert np.array_equal(got.view(np.uint32), serial.view(np.uint32)), (pool, tail)
