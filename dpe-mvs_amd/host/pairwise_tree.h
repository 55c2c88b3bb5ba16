// pairwise_tree.h — the pairwise sum in index order of include/dpe_mvs.h (dpe_cloud_icp_step, dpe_depth_score) taken
// literally on the host, K series at once, leaf by leaf.  lvl[l] holds the finished node of 2^l leaves that waits for
// its right sibling, exactly as a binary counter holds its digits, so push() forms the nodes
// s[k] = s_l[2k] + s_l[2k + 1] of every complete pair and finish() pads the ragged end with +0.0 level by level: the
// tree of the contract, node for node, without keeping its levels.
#pragma once

namespace dpe_host {

template <int K>
struct PairwiseTree {
  double lvl[64][K];
  unsigned long long n = 0;
  void push(const double* t) {
    double carry[K];
    for (int k = 0; k < K; ++k) carry[k] = t[k];
    int l = 0;
    for (unsigned long long c = n; c & 1ull; c >>= 1, ++l)
      for (int k = 0; k < K; ++k) carry[k] = lvl[l][k] + carry[k];
    for (int k = 0; k < K; ++k) lvl[l][k] = carry[k];
    ++n;
  }
  void finish(double* out) const {
    for (int k = 0; k < K; ++k) out[k] = 0.0;
    if (n == 0) return;
    bool have = false;   // out holds the ragged last node of the level
    for (int l = 0;; ++l) {
      const unsigned long long full = n >> l;             // complete nodes of 2^l leaves
      if (full + (have ? 1 : 0) == 1) {                   // one node left: the result
        if (!have)
          for (int k = 0; k < K; ++k) out[k] = lvl[l][k];
        return;
      }
      if (full & 1ull) {                                  // an odd complete node: its right is the ragged one, or +0.0
        for (int k = 0; k < K; ++k) out[k] = lvl[l][k] + (have ? out[k] : 0.0);
        have = true;
      } else if (have) {                                  // the ragged node has no right sibling
        for (int k = 0; k < K; ++k) out[k] = out[k] + 0.0;
      }
    }
  }
};

}  // namespace dpe_host
