// cloud_eval.cpp — the cloud evaluation on the host: the truncated nearest-neighbour distance of
// dpe_cloud_nn (include/dpe_mvs.h states the contract) over the same hashed grid (csrc/cloud_dist.h: the
// arithmetic, the cells and why 27 of them are enough) on host threads, with the nearest point's index when it
// is asked for (dpe_cloud_nn_index; the grid is a CloudIndex, cloud_index.h), and precision / recall / F-score
// from the two directions.  The yardstick of the device path and what runs without a GPU; no counterpart in
// the reference.  The counts and the means are taken on the host, in index order, from the distance arrays
// of either path, so both paths fill equal structs.
#include "host.h"
#include "cloud_index.h"
#include "parallel.h"

#include <atomic>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

namespace dpe_host {

using dpe::CloudGrid;

bool cloud_radius_ok(float radius) { return std::isfinite(radius) && radius > 0.0f; }

// The target's grid, built once and queried many times (one ICP stage builds it once for all its steps).
bool CloudIndex::build(const float* target, size_t m, float radius, const char* who, std::string& err) {
  r2 = radius * radius;
  // bounds of the finite target points
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  finite = 0;
  for (size_t j = 0; j < m; ++j) {
    const float* t = target + 3 * j;
    if (!dpe::cloud_finite3(t[0], t[1], t[2])) continue;
    for (int a = 0; a < 3; ++a) {
      if (!finite || t[a] < lo[a]) lo[a] = t[a];
      if (!finite || t[a] > hi[a]) hi[a] = t[a];
    }
    ++finite;
  }
  for (int a = 0; a < 3; ++a) origin[a] = (double)lo[a];
  if (finite == 0) return true;
  if (!dpe::cloud_grid_make(lo, hi, finite, radius, &g)) {
    err = std::string(who) + ": radius too small for the cloud's extent";
    return false;
  }
  // count, scan, fill: the target's points in bucket order, each with its original index
  const size_t nb = (size_t)g.mask + 1;
  end.assign(nb, 0);
  std::vector<uint32_t> bucket(m);
  for (size_t j = 0; j < m; ++j) {
    const float* t = target + 3 * j;
    if (!dpe::cloud_finite3(t[0], t[1], t[2])) { bucket[j] = UINT32_MAX; continue; }
    bucket[j] = dpe::cloud_bucket_of(g, t[0], t[1], t[2]);
    ++end[bucket[j]];
  }
  int run = 0;
  for (size_t b = 0; b < nb; ++b) { const int c = end[b]; end[b] = run; run += c; }
  st.resize(3 * finite);
  sj.resize(finite);
  for (size_t j = 0; j < m; ++j) {
    if (bucket[j] == UINT32_MAX) continue;
    const size_t slot = (size_t)end[bucket[j]]++;
    float* d = st.data() + 3 * slot;
    d[0] = target[3 * j]; d[1] = target[3 * j + 1]; d[2] = target[3 * j + 2];
    sj[slot] = (int32_t)j;
  }
  return true;
}

// out[i] (and idx[i] when idx is not null) of queries [i0, i1)
template <bool kIndex>
static void cloud_query_range(const CloudIndex& ix, const float* query, size_t i0, size_t i1, float* out, int32_t* idx) {
  const CloudGrid& g = ix.g;
  const int32_t top[3] = {(int32_t)g.hi[0], (int32_t)g.hi[1], (int32_t)g.hi[2]};
  for (size_t i = i0; i < i1; ++i) {
    const float qx = query[3 * i], qy = query[3 * i + 1], qz = query[3 * i + 2];
    float best = ix.r2;
    int best_j = -1;
    if (dpe::cloud_finite3(qx, qy, qz)) {
      const int32_t c[3] = {dpe::cloud_cell(qx, g.o[0], g.h, g.hi[0]), dpe::cloud_cell(qy, g.o[1], g.h, g.hi[1]),
                            dpe::cloud_cell(qz, g.o[2], g.h, g.hi[2])};
      for (int dz = -1; dz <= 1; ++dz) {
        const int32_t iz = c[2] + dz;
        if (iz < 0 || iz > top[2]) continue;
        for (int dy = -1; dy <= 1; ++dy) {
          const int32_t iy = c[1] + dy;
          if (iy < 0 || iy > top[1]) continue;
          for (int dx = -1; dx <= 1; ++dx) {
            const int32_t ixx = c[0] + dx;
            if (ixx < 0 || ixx > top[0]) continue;
            const uint32_t b = dpe::cloud_bucket(ixx, iy, iz, g.mask);
            const int j1 = ix.end[b];
            for (int j = b ? ix.end[b - 1] : 0; j < j1; ++j) {
              const float* t = ix.st.data() + 3 * (size_t)j;
              const float s = dpe::cloud_d2(qx, qy, qz, t[0], t[1], t[2]);
              if (kIndex) dpe::icp_take(s, ix.sj[(size_t)j], best, best_j);
              else best = s < best ? s : best;
            }
          }
        }
      }
    }
    out[i] = best;
    if (kIndex) idx[i] = best_j;
  }
}

void CloudIndex::query(const float* query, size_t n, float* out, int32_t* idx) const {
  if (finite == 0) {
    for (size_t i = 0; i < n; ++i) { out[i] = r2; if (idx) idx[i] = -1; }
    return;
  }
  // the queries in chunks handed out to the threads
  const size_t kChunk = 1024;
  const size_t chunks = (n + kChunk - 1) / kChunk;
  std::atomic<size_t> next{0};
  run_on_threads((int)std::min<size_t>((size_t)host_threads(), chunks), [&](int) {
    for (size_t ch = next++; ch < chunks; ch = next++) {
      const size_t i0 = ch * kChunk, i1 = std::min(n, (ch + 1) * kChunk);
      if (idx) cloud_query_range<true>(*this, query, i0, i1, out, idx);
      else cloud_query_range<false>(*this, query, i0, i1, out, idx);
    }
  });
}

static bool cloud_nn_any(const float* query, size_t n, const float* target, size_t m, float radius, float* out, int32_t* idx,
                         bool want_idx, const char* who, std::string& err) {
  if (n > (size_t)INT_MAX || m > (size_t)INT_MAX || (!query && n) || (!target && m) || (!out && n) || (want_idx && !idx && n) ||
      !cloud_radius_ok(radius)) {
    err = std::string(who) + ": bad argument";
    return false;
  }
  if (n == 0) return true;
  CloudIndex ix;
  if (!ix.build(target, m, radius, who, err)) return false;
  ix.query(query, n, out, idx);
  return true;
}

bool cloud_nn(const float* query, size_t n, const float* target, size_t m, float radius, float* out, std::string& err) {
  return cloud_nn_any(query, n, target, m, radius, out, nullptr, false, "cloud_nn", err);
}

bool cloud_nn_index(const float* query, size_t n, const float* target, size_t m, float radius, float* out, int32_t* idx,
                    std::string& err) {
  return cloud_nn_any(query, n, target, m, radius, out, idx, true, "cloud_nn_index", err);
}

namespace {

size_t count_nonfinite(const float* p, size_t n) {
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) k += dpe::cloud_finite3(p[3 * i], p[3 * i + 1], p[3 * i + 2]) ? 0 : 1;
  return k;
}

// the share of d2[0..n) below tau^2 (the product in float, the division in double) and the truncated mean
void cloud_stats(const float* d2, size_t n, const float* tau, int n_tau, double* share, double* mean) {
  double sum = 0.0;
  for (size_t i = 0; i < n; ++i) sum += std::sqrt((double)d2[i]);
  *mean = n ? sum / (double)n : 0.0;
  for (int k = 0; k < n_tau; ++k) {
    const float t2 = tau[k] * tau[k];
    size_t hit = 0;
    for (size_t i = 0; i < n; ++i) hit += d2[i] < t2 ? 1 : 0;
    share[k] = n ? (double)hit / (double)n : 0.0;
  }
}

}  // namespace

// what cloud_eval refuses before any work, and the radius R it uses
static bool cloud_eval_args(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                            const DpeCloudEval* out, float* R_out, std::string& err) {
  if (!out || !tau || n_tau < 1 || n_tau > DPE_CLOUD_MAX_TAU) { err = "cloud_eval: 1 to 16 thresholds expected"; return false; }
  if (n > (size_t)INT_MAX || m > (size_t)INT_MAX || (!recon && n) || (!gt && m)) { err = "cloud_eval: bad cloud"; return false; }
  float tmax = 0.0f;
  for (int k = 0; k < n_tau; ++k) {
    if (!(std::isfinite(tau[k]) && tau[k] > 0.0f)) { err = "cloud_eval: a threshold is not a finite positive number"; return false; }
    tmax = std::max(tmax, tau[k]);
  }
  const float R = radius == 0.0f ? tmax : radius;
  if (!cloud_radius_ok(R)) { err = "cloud_eval: the radius is not a finite positive number"; return false; }
  if (tmax > R) { err = "cloud_eval: a threshold exceeds the radius"; return false; }
  *R_out = R;
  return true;
}

bool cloud_eval_in(DpeContext* ctx, const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau,
                   float radius, DpeCloudEval* out, std::string& err) {
  float R = 0.0f;
  if (!cloud_eval_args(recon, n, gt, m, tau, n_tau, radius, out, &R, err)) return false;
  std::vector<float> a(n), c(m);
  if (!ctx) {
    if (!cloud_nn(recon, n, gt, m, R, a.data(), err) || !cloud_nn(gt, m, recon, n, R, c.data(), err)) return false;
  } else if (dpe_cloud_nn_pair(ctx, recon, n, gt, m, R, a.data(), c.data()) != 0) {
    err = std::string("cloud_eval: ") + dpe_last_error();
    return false;
  }
  *out = DpeCloudEval{};
  out->n_tau = n_tau;
  out->radius = R;
  for (int k = 0; k < n_tau; ++k) out->tau[k] = tau[k];
  out->n_recon = n;
  out->n_gt = m;
  out->dropped_recon = count_nonfinite(recon, n);
  out->dropped_gt = count_nonfinite(gt, m);
  cloud_stats(a.data(), n, tau, n_tau, out->precision, &out->mean_accuracy_truncated);
  cloud_stats(c.data(), m, tau, n_tau, out->recall, &out->mean_completeness_truncated);
  for (int k = 0; k < n_tau; ++k) {
    const double p = out->precision[k], r = out->recall[k];
    out->fscore[k] = p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0;
  }
  return true;
}

bool cloud_eval(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                int gpu_index, DpeCloudEval* out, std::string& err) {
  float R = 0.0f;
  if (!cloud_eval_args(recon, n, gt, m, tau, n_tau, radius, out, &R, err)) return false;   // before a context is made
  OwnedContext own(gpu_index, "cloud_eval", err);
  return own.ok && cloud_eval_in(own.ctx, recon, n, gt, m, tau, n_tau, radius, out, err);
}

}  // namespace dpe_host

extern "C" {

int dpe_host_cloud_nn(const float* query, size_t n, const float* target, size_t m, float radius, float* d2_out) {
  return dpe_host::c_entry([&](std::string& err) { return dpe_host::cloud_nn(query, n, target, m, radius, d2_out, err); });
}

int dpe_host_cloud_nn_index(const float* query, size_t n, const float* target, size_t m, float radius, float* d2_out,
                            int32_t* idx_out) {
  return dpe_host::c_entry([&](std::string& err) { return dpe_host::cloud_nn_index(query, n, target, m, radius, d2_out, idx_out, err); });
}

int dpe_host_cloud_eval(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                        int gpu_index, DpeCloudEval* out) {
  return dpe_host::c_entry([&](std::string& err) { return dpe_host::cloud_eval(recon, n, gt, m, tau, n_tau, radius, gpu_index, out, err); });
}

}  // extern "C"
