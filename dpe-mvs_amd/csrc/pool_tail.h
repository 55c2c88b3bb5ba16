// pool_tail.h — the lane map of a split last round of the strong sweep's job pools.
//
// A pool deals its jobs (one 36-tap NCC each) round-robin over the 64 lanes.  When the last round
// holds only `tail` <= kTailMaxJobs jobs, each of them is split by patch rows over several lanes:
//   tail  1..10   6 lanes per job, 1 row each
//   tail 11..16   3 lanes per job, 2 rows each
//   tail 17..32   2 lanes per job, 3 rows each
//   larger        not split (one lane per job, all 6 rows)
// A job's lanes are adjacent and take ascending, contiguous rows.  The NCC sums are the row
// triplets added to zero in row order, so the split keeps that association: the first lane of a
// job starts from zero, a lane that continues a job adds its rows, in order, to the partial it is
// handed, and the job's last lane finishes the NCC.  Both pools (cost vectors, refinement) use
// this one map.  Plain C++ (no HIP types): the CPU tests compile it with g++.
#pragma once

#if defined(__HIPCC__)
#define TAIL_HD __host__ __device__
#else
#define TAIL_HD
#endif

namespace dpe {

constexpr int kTailMaxJobs = 32;    // the largest last round that is split
constexpr int kTailLdsJobs = 16;    // up to here every row triplet of a job has its own LDS slot

// lanes that share one job of a last round of `tail` jobs (1: the round is not split)
TAIL_HD constexpr int tail_lanes_per_job(int tail) {
  return tail <= 10 ? 6 : tail <= kTailLdsJobs ? 3 : tail <= kTailMaxJobs ? 2 : 1;
}

struct TailLane {
  int job;     // index within the last round, 0..tail-1 (-1: the lane has no work)
  int row0;    // first patch row
  int rows;    // row count
  bool last;   // the job's last lane: it ends the chain of partial sums
};

TAIL_HD constexpr TailLane tail_lane(int tail, int lane) {
  const int npc = tail_lanes_per_job(tail), rpl = 6 / npc;
  if (lane >= tail * npc) return TailLane{-1, 0, 0, false};
  return TailLane{lane / npc, (lane % npc) * rpl, rpl, lane % npc == npc - 1};
}

// Float slot of row `a` of job `job` in the pools' LDS tail region (kTailLdsJobs * 18 floats).
// Up to kTailLdsJobs jobs: all six triplets, [job][row][3].  With two lanes per job only the second
// lane's rows 3..5 go through LDS, [job][row - 3][3] (32 * 9 floats, the same region); the first
// lane's partial is handed over by a lane shuffle.
TAIL_HD constexpr int tail_lds_slot(int tail, int job, int a) {
  return tail_lanes_per_job(tail) == 2 ? (job * 3 + (a - 3)) * 3 : (job * 6 + a) * 3;
}

}  // namespace dpe
