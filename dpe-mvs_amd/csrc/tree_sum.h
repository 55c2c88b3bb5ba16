// tree_sum.h — the pairwise tree of include/dpe_mvs.h (DpeIcpSums, DpeDepthScore) on the device: K doubles per
// leaf, 256 consecutive leaves per block, level by level until one block's result is left.
//
// The butterfly.  At level o = 1, 2, .. 32 a lane adds its partner's value (lane ^ o) to its own; addition is
// commutative, so both lanes of a pair hold the node s[2k] + s[2k + 1] of the contract's tree, and lanes past the
// end hold +0.0, the tree's missing right operand.  Two more levels go over the four waves through LDS as
// (w0 + w1) + (w2 + w3).  256 consecutive leaves are a complete subtree, so the levels over the block results
// (k_tree_reduce) continue the same tree.  No float atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

namespace dpe {

constexpr int kTreeBlock = 256;   // the leaves of a block; the kernels that feed the tree use blocks of this size

// a double from lane ^ o, moved as its two halves
__device__ inline double shfl_xor_double(double v, int o) {
  const int lo = __shfl_xor(__double2loint(v), o), hi = __shfl_xor(__double2hiint(v), o);
  return __hiloint2double(hi, lo);
}

// t[0..K) of the 256 threads of a block summed by the butterfly; threads 0..K-1 write the K sums to out.  Its
// barrier also publishes what the caller wrote to LDS before it
template <int K>
__device__ inline void block_tree_sum(double* t, double* __restrict__ out) {
  __shared__ double part[kTreeBlock / 64][K];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = t[k] + shfl_xor_double(t[k], o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) part[wave][k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    const double left = part[0][k] + part[1][k], right = part[2][k] + part[3][k];
    out[k] = left + right;
  }
}

// in: cnt partials of K doubles; out: one per block of 256 of them
template <int K>
__global__ void __launch_bounds__(kTreeBlock) k_tree_reduce(const double* __restrict__ in, size_t cnt, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kTreeBlock + threadIdx.x;
  double t[K];
#pragma unroll
  for (int k = 0; k < K; ++k) t[k] = i < cnt ? in[i * K + k] : 0.0;
  block_tree_sum<K>(t, out + (size_t)blockIdx.x * K);
}

}  // namespace dpe
