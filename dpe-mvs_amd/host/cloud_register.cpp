// cloud_register.cpp — rigid registration of point clouds on the host: one step of point-to-point ICP as
// include/dpe_mvs.h states it (dpe_cloud_icp_step), with the pairwise tree taken literally, the solve for the
// transform (Horn's unit quaternion by cyclic Jacobi) and the loop over a schedule of radii.  The step is the
// yardstick of the device step and what runs without a GPU; the solve and the loop are written once, here, and
// both paths go through them, so both fill equal structs.  The arithmetic of a step is csrc/cloud_reg.h's, which
// the kernels (csrc/pass_register.h) share.  No counterpart in the reference.
#include "host.h"
#include "cloud_index.h"
#include "pairwise_tree.h"

#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace dpe_host {

namespace {

using dpe::kIcpTerms;

void cloud_minima(const float* p, size_t n, double* o) {
  bool any = false;
  o[0] = o[1] = o[2] = 0.0;
  for (size_t i = 0; i < n; ++i) {
    const float* q = p + 3 * i;
    if (!dpe::cloud_finite3(q[0], q[1], q[2])) continue;
    for (int a = 0; a < 3; ++a)
      if (!any || (double)q[a] < o[a]) o[a] = (double)q[a];
    any = true;
  }
}

void cloud_transform(const double* T, const float* xyz, size_t n, float* out) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (size_t i = 0; i < n; ++i) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (dpe::cloud_finite3(x, y, z)) dpe::icp_apply(T, x, y, z, out + 3 * i);
    else out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = nan;
  }
}

// one step over a built target index: the transformed source, the match, the 16 sums and the count
void icp_step_over(const CloudIndex& ix, const float* src, size_t n, const float* tgt, const double* o_s, const double* T,
                   std::vector<float>& moved, std::vector<float>& d2, std::vector<int32_t>& idx, DpeIcpSums* out) {
  moved.resize(3 * n);
  d2.resize(n);
  idx.resize(n);
  cloud_transform(T, src, n, moved.data());
  ix.query(moved.data(), n, d2.data(), idx.data());
  PairwiseTree<kIcpTerms> tree;
  long long matched = 0;
  const double zero[kIcpTerms] = {0};
  for (size_t i = 0; i < n; ++i) {
    if (idx[i] < 0) { tree.push(zero); continue; }
    double t[kIcpTerms];
    dpe::icp_terms(src + 3 * i, tgt + 3 * (size_t)idx[i], d2[i], o_s, ix.origin, t);
    tree.push(t);
    ++matched;
  }
  double s[kIcpTerms];
  tree.finish(s);
  out->matched = matched;
  out->d2 = s[0];
  for (int k = 0; k < 3; ++k) { out->a[k] = s[1 + k]; out->b[k] = s[4 + k]; }
  for (int k = 0; k < 9; ++k) out->ab[k] = s[7 + k];
}

bool icp_clouds_ok(const float* src, size_t n, const float* tgt, size_t m) {
  return n <= (size_t)INT_MAX && m <= (size_t)INT_MAX && (src || n == 0) && (tgt || m == 0);
}

// cyclic Jacobi on a symmetric 4 x 4 matrix: A becomes diagonal, V's columns the eigenvectors; sqrt only
void jacobi4(double A[4][4], double V[4][4]) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 4; ++p)
      for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
    if (off == 0.0) return;
    for (int p = 0; p < 4; ++p) {
      for (int q = p + 1; q < 4; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double mag = theta < 0.0 ? -theta : theta;
        double t = 1.0 / (mag + std::sqrt(theta * theta + 1.0));   // theta^2 = inf gives t = 0
        if (theta < 0.0) t = -t;
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {                              // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {                              // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
    }
  }
}

}  // namespace

bool cloud_icp_step(const float* src, size_t n, const float* tgt, size_t m, float radius, const double* T, DpeIcpSums* out,
                    std::string& err) {
  if (!icp_clouds_ok(src, n, tgt, m) || !cloud_radius_ok(radius) || !T || !out) {
    err = "cloud_icp_step: bad argument";
    return false;
  }
  CloudIndex ix;
  if (!ix.build(tgt, m, radius, "cloud_icp_step", err)) return false;
  double o_s[3];
  cloud_minima(src, n, o_s);
  std::vector<float> moved, d2;
  std::vector<int32_t> idx;
  DpeIcpSums s;
  icp_step_over(ix, src, n, tgt, o_s, T, moved, d2, idx, &s);
  *out = s;
  return true;
}

bool cloud_solve(const DpeIcpSums& s, const double* o_s, const double* o_t, double* T, std::string& err) {
  if (s.matched < 3) {
    err = "cloud_register: fewer than 3 matches within the radius";
    return false;
  }
  const double N = (double)s.matched;
  double ma[3], mb[3], H[3][3];
  for (int k = 0; k < 3; ++k) { ma[k] = s.a[k] / N; mb[k] = s.b[k] / N; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) H[r][c] = s.ab[3 * r + c] - s.a[r] * s.b[c] / N;
  // Horn's matrix of H (H[r][c] = sum of a_r b_c, a the source): its top eigenvector is the quaternion (w, x, y, z)
  // of the rotation that takes a to b
  double A[4][4] = {
      {H[0][0] + H[1][1] + H[2][2], H[1][2] - H[2][1], H[2][0] - H[0][2], H[0][1] - H[1][0]},
      {H[1][2] - H[2][1], H[0][0] - H[1][1] - H[2][2], H[0][1] + H[1][0], H[2][0] + H[0][2]},
      {H[2][0] - H[0][2], H[0][1] + H[1][0], -H[0][0] + H[1][1] - H[2][2], H[1][2] + H[2][1]},
      {H[0][1] - H[1][0], H[2][0] + H[0][2], H[1][2] + H[2][1], -H[0][0] - H[1][1] + H[2][2]}};
  double V[4][4];
  jacobi4(A, V);
  int top = 0;
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > A[top][top]) top = k;
  double q[4] = {V[0][top], V[1][top], V[2][top], V[3][top]};
  const double len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!(len > 0.0) || !std::isfinite(len)) {
    err = "cloud_register: the sums are not finite";
    return false;
  }
  for (double& v : q) v /= len;
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                          {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                          {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
  for (int r = 0; r < 3; ++r) {
    double moved = 0.0;
    for (int c = 0; c < 3; ++c) {
      T[4 * r + c] = R[r][c];
      moved += R[r][c] * (o_s[c] + ma[c]);
    }
    T[4 * r + 3] = (o_t[r] + mb[r]) - moved;
  }
  return true;
}

static bool register_args(const float* src, size_t n, const float* tgt, size_t m, const DpeCloudRegOptions* opt, const DpeCloudReg* out,
                          std::string& err) {
  if (!opt || !out || !icp_clouds_ok(src, n, tgt, m)) { err = "cloud_register: bad argument"; return false; }
  if (opt->n_radii < 1 || opt->n_radii > DPE_CLOUD_MAX_RADII) { err = "cloud_register: 1 to 4 radii expected"; return false; }
  for (int k = 0; k < opt->n_radii; ++k)
    if (!cloud_radius_ok(opt->radius[k])) { err = "cloud_register: a radius is not a finite positive number"; return false; }
  if (opt->max_iters < 1 || opt->max_iters > 1000) { err = "cloud_register: 1 to 1000 iterations expected"; return false; }
  if (!(opt->tol >= 0.0)) { err = "cloud_register: the tolerance is negative or not a number"; return false; }
  if (opt->use_init)
    for (double v : opt->init)
      if (!std::isfinite(v)) { err = "cloud_register: the initial transform is not finite"; return false; }
  return true;
}

bool cloud_register_in(DpeContext* ctx, const float* src, size_t n, const float* tgt, size_t m, const DpeCloudRegOptions& opt,
                       DpeCloudReg* out, std::string& err) {
  if (!register_args(src, n, tgt, m, &opt, out, err)) return false;
  DpeCloudReg reg{};
  const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  std::memcpy(reg.T, opt.use_init ? opt.init : identity, sizeof reg.T);
  reg.stages = opt.n_radii;
  double o_s[3], o_t[3];
  cloud_minima(src, n, o_s);
  cloud_minima(tgt, m, o_t);
  std::vector<float> moved, d2;
  std::vector<int32_t> idx;
  for (int st = 0; st < opt.n_radii; ++st) {
    const float radius = opt.radius[st];
    CloudIndex ix;
    if (!ctx) {
      if (!ix.build(tgt, m, radius, "cloud_register", err)) return false;
    } else if (dpe_cloud_icp_stage(ctx, src, n, tgt, m, radius) != 0) {
      err = device_error("cloud_register", "dpe_cloud_icp_stage");
      return false;
    }
    DpeIcpSums prev{};
    double rms_prev = 0.0;
    for (int it = 1; it <= opt.max_iters; ++it) {
      DpeIcpSums s;
      std::memset(&s, 0, sizeof s);   // the structs are compared as bytes
      if (!ctx) {
        icp_step_over(ix, src, n, tgt, o_s, reg.T, moved, d2, idx, &s);
      } else if (dpe_cloud_icp_step(ctx, reg.T, &s) != 0) {
        err = std::string("cloud_register: ") + dpe_last_error();
        return false;
      }
      if (!cloud_solve(s, o_s, o_t, reg.T, err)) return false;
      const double rms = std::sqrt(s.d2 / (double)s.matched);
      reg.iters[st] = it;
      reg.matched[st] = s.matched;
      reg.rms[st] = rms;
      reg.converged[st] = 0;
      if (it > 1 && std::memcmp(&s, &prev, sizeof s) == 0) { reg.converged[st] = 2; break; }
      const double change = rms > rms_prev ? rms - rms_prev : rms_prev - rms;
      if (it > 1 && change <= opt.tol * rms_prev) { reg.converged[st] = 1; break; }
      prev = s;
      rms_prev = rms;
    }
  }
  *out = reg;
  return true;
}

static bool cloud_register(const float* src, size_t n, const float* tgt, size_t m, const DpeCloudRegOptions* opt, int gpu_index,
                           DpeCloudReg* out, std::string& err) {
  if (!register_args(src, n, tgt, m, opt, out, err)) return false;   // before a context is made
  OwnedContext own(gpu_index, "cloud_register", err);
  return own.ok && cloud_register_in(own.ctx, src, n, tgt, m, *opt, out, err);
}

static bool cloud_eval_reg(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                           int gpu_index, DpeCloudPrep* prep, const DpeCloudRegOptions* opt, DpeCloudReg* reg, DpeCloudEval* out,
                           std::string& err) {
  if (!register_args(recon, n, gt, m, opt, reg, err)) return false;
  const DpeCloudPrep none{};
  if (!cloud_prep_args(recon, n, gt, m, prep ? *prep : none, err)) return false;
  OwnedContext own(gpu_index, "cloud_eval", err);
  if (!own.ok) return false;
  DpeContext* ctx = own.ctx;
  // what is registered: the reconstruction down-sampled but never cropped (the box is in the ground truth's frame),
  // the ground truth as it will be scored
  std::vector<float> a, b, moved(3 * n);
  DpeCloudReg r;
  DpeCloudPrep scratch = prep ? *prep : none;
  bool ok = cloud_prepare(ctx, recon, n, scratch, false, a, err) && cloud_prepare(ctx, gt, m, scratch, scratch.use_crop != 0, b, err) &&
            cloud_register_in(ctx, a.data(), a.size() / 3, b.data(), b.size() / 3, *opt, &r, err);
  if (ok) {
    cloud_transform(r.T, recon, n, moved.data());
    ok = prep ? cloud_eval_prep_in(ctx, moved.data(), n, gt, m, tau, n_tau, radius, prep, out, err)
              : cloud_eval_in(ctx, moved.data(), n, gt, m, tau, n_tau, radius, out, err);
  }
  if (ok) *reg = r;
  return ok;
}

}  // namespace dpe_host

extern "C" {

int dpe_host_cloud_icp_step(const float* src, size_t n, const float* tgt, size_t m, float radius, const double* T,
                            DpeIcpSums* out) {
  return dpe_host::c_entry([&](std::string& err) { return dpe_host::cloud_icp_step(src, n, tgt, m, radius, T, out, err); });
}

int dpe_host_cloud_transform(const double* T, const float* xyz, size_t n, float* out) {
  if (!T || n > (size_t)INT_MAX || (n && (!xyz || !out))) {
    dpe_host::set_last_error("cloud_transform: bad argument");
    return 1;
  }
  dpe_host::cloud_transform(T, xyz, n, out);
  return 0;
}

int dpe_host_cloud_solve(const DpeIcpSums* sums, const double* o_s, const double* o_t, double* T) {
  return dpe_host::c_entry([&](std::string& err) { return sums && o_s && o_t && T && dpe_host::cloud_solve(*sums, o_s, o_t, T, err); },
                           "cloud_solve: bad argument");
}

int dpe_host_cloud_register(const float* src, size_t n, const float* tgt, size_t m, const DpeCloudRegOptions* opt, int gpu_index,
                            DpeCloudReg* out) {
  return dpe_host::c_entry([&](std::string& err) { return dpe_host::cloud_register(src, n, tgt, m, opt, gpu_index, out, err); });
}

int dpe_host_cloud_eval_reg(const float* recon, size_t n, const float* gt, size_t m, const float* tau, int n_tau, float radius,
                            int gpu_index, DpeCloudPrep* prep, const DpeCloudRegOptions* opt, DpeCloudReg* reg, DpeCloudEval* out) {
  return dpe_host::c_entry(
      [&](std::string& err) { return dpe_host::cloud_eval_reg(recon, n, gt, m, tau, n_tau, radius, gpu_index, prep, opt, reg, out, err); });
}

}  // extern "C"
