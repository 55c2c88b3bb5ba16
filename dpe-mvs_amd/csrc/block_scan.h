// block_scan.h — the one scan over a 256-thread block: a __shfl_up ladder within each wave, the four wave totals
// through LDS.  For an associative operation on int; + and max are what the kernels need (the offsets of the
// compactions, the last-valid carry of pass_fusion_tat.h).  No scratch, and the order of the combinations is fixed,
// so the result does not depend on the schedule.
#pragma once
#include <hip/hip_runtime.h>

namespace dpe {

constexpr int kScanBlock = 256;   // the threads of a block that scans

struct ScanSum {
  static __device__ inline int op(int a, int b) { return a + b; }
};
struct ScanMax {
  static __device__ inline int op(int a, int b) { return max(a, b); }
};

// Inclusive scan of v over the block's threads (all of them call it); *all = the combination of the whole block.
// s4: four ints of LDS the caller provides; free again when the call returns.
template <class Op>
__device__ inline int block_scan(int v, int* s4, int* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl = Op::op(incl, t);
  }
  if (lane == 63) s4[wave] = incl;
  __syncthreads();
  const int w0 = s4[0], w1 = s4[1], w2 = s4[2], w3 = s4[3];   // read at once: a single block's scan waits on nothing else
  if (wave > 0) incl = Op::op(incl, w0);
  if (wave > 1) incl = Op::op(incl, w1);
  if (wave > 2) incl = Op::op(incl, w2);
  *all = Op::op(Op::op(w0, w1), Op::op(w2, w3));
  __syncthreads();
  return incl;
}

// Exclusive sum-scan of cnt[0..n) in place by one block (<<<1, kScanBlock>>>), tile by tile with a carry: counts
// become offsets, and their total goes into *tot.  A template, so that only the units that launch it hold a copy;
// kThreads is the launch's block.
template <int kThreads>
__global__ void __launch_bounds__(kThreads) k_offsets_scan(int n, int* __restrict__ cnt, int* __restrict__ tot) {
  static_assert(kThreads == kScanBlock, "block_scan scans 256 threads");
  __shared__ int s4[4];
  int acc = 0;   // the total of the tiles before this one
  for (int k0 = 0; k0 < n; k0 += kScanBlock) {
    const int k = k0 + (int)threadIdx.x;
    const int c = k < n ? cnt[k] : 0;
    int all;
    const int incl = block_scan<ScanSum>(c, s4, &all);
    if (k < n) cnt[k] = acc + incl - c;
    acc += all;
  }
  if (threadIdx.x == 0) *tot = acc;
}

}  // namespace dpe
