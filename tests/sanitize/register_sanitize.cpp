// Drives the host registration (host/cloud_register.cpp over the grid of host/cloud_eval.cpp) under ASan + UBSan
// (tests/test_cloud_register.py): one ICP step at n = 1, 257 and 65 537 into exactly sized heap buffers, compared
// bit for bit with a literal pairwise tree over terms formed here from the index call's matches; the loop on the wavy
// sheet of the Python test (a known motion, one and two stages); the transform; and every refusal, which must leave
// its output alone.  Linked with those sources and host/ply_read.cpp only: the few symbols of the other libraries they
// refer to are defined here (no device path, no voxels in this program).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "no_device.h"

// ---- what host/cloud_voxel.cpp provides in the library, and the device entries of these sources (no_device.h: the rest)
namespace dpe_host {
bool cloud_prep_args(const float*, size_t, const float*, size_t, const DpeCloudPrep&, std::string&) { return true; }
bool cloud_prepare(DpeContext*, const float* xyz, size_t n, const DpeCloudPrep&, bool, std::vector<float>& pts, std::string&) {
  pts.assign(xyz, xyz + 3 * n);   // no voxels and no crop in this program
  return true;
}
bool cloud_eval_prep_in(DpeContext*, const float*, size_t, const float*, size_t, const float*, int, float, DpeCloudPrep*, DpeCloudEval*,
                        std::string& err) {
  err = "no preparation in this program";
  return false;
}
}  // namespace dpe_host
extern "C" int dpe_cloud_nn_pair(DpeContext*, const float*, size_t, const float*, size_t, float, float*, float*) { return DPE_ERR_ARG; }
extern "C" int dpe_cloud_icp_stage(DpeContext*, const float*, size_t, const float*, size_t, float) { return DPE_ERR_ARG; }
extern "C" int dpe_cloud_icp_step(DpeContext*, const double*, DpeIcpSums*) { return DPE_ERR_ARG; }

static int fail(const std::string& what) {
  std::fprintf(stderr, "register sanitize: %s (last error: %s)\n", what.c_str(), g_msg.c_str());
  return 1;
}

static unsigned g_seed = 20261020u;
static double rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (double)(g_seed >> 8) / 16777216.0; }

// the contract's tree, literally: level by level over all the terms
static void literal_tree(std::vector<double> s, size_t n, double* out) {
  while (n > 1) {
    const size_t half = (n + 1) / 2;
    for (size_t k = 0; k < half; ++k)
      for (int c = 0; c < 16; ++c) s[16 * k + c] = s[16 * (2 * k) + c] + (2 * k + 1 < n ? s[16 * (2 * k + 1) + c] : 0.0);
    n = half;
  }
  for (int c = 0; c < 16; ++c) out[c] = n ? s[c] : 0.0;
}

// one step on the first n sources against its own restatement: transform, index call, terms, literal tree
static int run_step(const std::vector<float>& P, size_t n, const std::vector<float>& G, float R, const double* T) {
  const size_t m = G.size() / 3;
  float* src = new float[3 * n];              // exactly sized: a read past the end is a report
  std::memcpy(src, P.data(), 3 * n * sizeof(float));
  DpeIcpSums got;
  if (dpe_host_cloud_icp_step(src, n, G.data(), m, R, T, &got) != 0) return fail("step refused");
  float* moved = new float[3 * n];
  float* d2 = new float[n];
  int32_t* idx = new int32_t[n];
  if (dpe_host_cloud_transform(T, src, n, moved) != 0 || dpe_host_cloud_nn_index(moved, n, G.data(), m, R, d2, idx) != 0)
    return fail("transform / index refused");
  double os[3] = {0, 0, 0}, ot[3] = {0, 0, 0};
  bool any = false;
  for (size_t i = 0; i < n; ++i) {
    if (!(std::isfinite(src[3 * i]) && std::isfinite(src[3 * i + 1]) && std::isfinite(src[3 * i + 2]))) continue;
    for (int a = 0; a < 3; ++a) if (!any || (double)src[3 * i + a] < os[a]) os[a] = (double)src[3 * i + a];
    any = true;
  }
  for (size_t j = 0; j < m; ++j)
    for (int a = 0; a < 3; ++a) if (j == 0 || (double)G[3 * j + a] < ot[a]) ot[a] = (double)G[3 * j + a];
  std::vector<double> terms(16 * n, 0.0);
  long long matched = 0;
  for (size_t i = 0; i < n; ++i) {
    if (idx[i] < 0) continue;
    if ((size_t)idx[i] >= m) return fail("index out of range");
    ++matched;
    double* t = &terms[16 * i];
    double a[3], b[3];
    for (int r = 0; r < 3; ++r) { a[r] = (double)src[3 * i + r] - os[r]; b[r] = (double)G[3 * (size_t)idx[i] + r] - ot[r]; }
    t[0] = (double)d2[i];
    for (int r = 0; r < 3; ++r) { t[1 + r] = a[r]; t[4 + r] = b[r]; }
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t[7 + 3 * r + c] = a[r] * b[c];
  }
  double want[16];
  literal_tree(terms, n, want);
  const double have[16] = {got.d2, got.a[0], got.a[1], got.a[2], got.b[0], got.b[1], got.b[2], got.ab[0], got.ab[1], got.ab[2],
                           got.ab[3], got.ab[4], got.ab[5], got.ab[6], got.ab[7], got.ab[8]};
  if (got.matched != matched || std::memcmp(have, want, sizeof want) != 0) return fail("step at n = " + std::to_string(n));
  delete[] src; delete[] moved; delete[] d2; delete[] idx;
  return 0;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  // ---- the step: 2 000 targets in the unit cube; sources near targets, every third one lifted out of reach, a few
  // non-finite ones
  std::vector<float> G, P;
  for (int j = 0; j < 2000; ++j) for (int a = 0; a < 3; ++a) G.push_back((float)rnd());
  for (int i = 0; i < 65537; ++i) {
    const size_t j = (size_t)(rnd() * 2000.0) % 2000;
    for (int a = 0; a < 3; ++a) P.push_back(G[3 * j + a] + (float)((rnd() - 0.5) * 0.04) + (a == 2 && i % 3 == 1 ? 1.2f : 0.0f));
  }
  P[3 * 5] = nan; P[3 * 100 + 1] = inf; P[3 * 300 + 2] = -inf;
  const double c = std::cos(0.02), s = std::sin(0.02);
  const double turned[12] = {c, -s, 0, 0.004, s, c, 0, -0.003, 0, 0, 1, 0.002};
  for (size_t n : {(size_t)1, (size_t)257, (size_t)65537})
    if (run_step(P, n, G, 0.05f, identity) || run_step(P, n, G, 0.05f, turned)) return 1;
  {
    DpeIcpSums z;
    std::vector<float> none;
    if (dpe_host_cloud_icp_step(P.data(), 257, none.data(), 0, 0.05f, identity, &z) != 0 || z.matched != 0 || z.d2 != 0.0 || std::signbit(z.d2) ||
        std::signbit(z.ab[8]))
      return fail("empty target");
  }
  // ---- the loop: the wavy sheet, 1 500 of its 4 000 points moved by the inverse of a 4 degree turn about (1, 2, 3) and
  // a shift
  std::vector<float> S, Q;
  for (int j = 0; j < 4000; ++j) {
    const double x = rnd(), y = rnd();
    S.push_back((float)x); S.push_back((float)y);
    S.push_back((float)(0.1 * std::sin(3 * x) * std::cos(2 * y) + 0.05 * std::sin(11 * x + 1) * std::sin(7 * y)));
  }
  const double k[3] = {1 / std::sqrt(14.0), 2 / std::sqrt(14.0), 3 / std::sqrt(14.0)}, th = 4.0 * 3.14159265358979323846 / 180.0;
  const double K[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
  double R0[3][3];
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) {
      double kk = 0;
      for (int e = 0; e < 3; ++e) kk += K[r][e] * K[e][q];
      R0[r][q] = (r == q ? 1.0 : 0.0) + std::sin(th) * K[r][q] + (1 - std::cos(th)) * kk;
    }
  const double t0[3] = {0.03, -0.02, 0.01};
  for (int i = 0; i < 1500; ++i) {
    const float* g = &S[3 * (size_t)((i * 2654435761u) % 4000u)];
    for (int r = 0; r < 3; ++r) {          // R0^T (g - t0)
      double v = 0;
      for (int e = 0; e < 3; ++e) v += R0[e][r] * ((double)g[e] - t0[e]);
      Q.push_back((float)v);
    }
  }
  DpeCloudRegOptions opt{};
  opt.radius[0] = 0.15f; opt.n_radii = 1; opt.max_iters = 50; opt.tol = 1e-6;
  DpeCloudReg reg;
  if (dpe_host_cloud_register(Q.data(), 1500, S.data(), 4000, &opt, -1, &reg) != 0) return fail("loop refused");
  double worst = 0;
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) worst = std::fmax(worst, std::fabs(reg.T[4 * r + q] - R0[r][q]));
    worst = std::fmax(worst, std::fabs(reg.T[4 * r + 3] - t0[r]));
  }
  if (reg.stages != 1 || reg.converged[0] != 2 || reg.matched[0] != 1500 || !(worst < 1e-7)) return fail("loop, one stage");
  DpeCloudReg two;
  opt.radius[0] = 0.3f; opt.radius[1] = 0.05f; opt.n_radii = 2;
  if (dpe_host_cloud_register(Q.data(), 1500, S.data(), 4000, &opt, -1, &two) != 0 || two.stages != 2 || two.converged[1] != 2 ||
      two.matched[1] != 1500)
    return fail("loop, two stages");
  for (int e = 0; e < 12; ++e) if (std::fabs(two.T[e] - reg.T[e]) > 1e-9) return fail("the two schedules disagree");
  {  // the transform in place, exactly sized
    float* q = new float[3 * 1500];
    std::memcpy(q, Q.data(), 3 * 1500 * sizeof(float));
    if (dpe_host_cloud_transform(reg.T, q, 1500, q) != 0) return fail("transform");
    const float* g = &S[3 * (size_t)((7 * 2654435761u) % 4000u)];
    if (std::fabs(q[21] - g[0]) > 1e-6f || std::fabs(q[22] - g[1]) > 1e-6f || std::fabs(q[23] - g[2]) > 1e-6f) return fail("the source is not home");
    delete[] q;
  }
  // ---- refusals: each with its message, each leaving its output alone
  unsigned char mark[sizeof(DpeCloudReg)];
  std::memset(mark, 0x5A, sizeof mark);
  auto refused = [&](const char* what, const float* src, size_t n, const float* tgt, size_t m, const DpeCloudRegOptions& o, const char* needle) {
    DpeCloudReg out;
    std::memset(&out, 0x5A, sizeof out);
    g_msg.clear();
    if (dpe_host_cloud_register(src, n, tgt, m, &o, -1, &out) == 0) return fail(std::string(what) + ": accepted");
    if (g_msg.find(needle) == std::string::npos) return fail(std::string(what) + ": message without '" + needle + "'");
    if (std::memcmp(&out, mark, sizeof out) != 0) return fail(std::string(what) + ": output written");
    return 0;
  };
  opt.radius[0] = 0.15f; opt.n_radii = 1;
  std::vector<float> away(Q);
  for (float& v : away) v += 50.0f;
  if (refused("no match", away.data(), 1500, S.data(), 4000, opt, "fewer than 3 matches")) return 1;
  if (refused("two sources", Q.data(), 2, S.data(), 4000, opt, "fewer than 3 matches")) return 1;
  for (float bad : {0.0f, nan, inf, -1.0f}) {
    DpeCloudRegOptions o = opt;
    o.radius[0] = bad;
    if (refused("bad radius", Q.data(), 1500, S.data(), 4000, o, "radius is not a finite positive")) return 1;
  }
  for (int nr : {0, 5}) {
    DpeCloudRegOptions o = opt;
    o.n_radii = nr;
    if (refused("number of radii", Q.data(), 1500, S.data(), 4000, o, "1 to 4 radii")) return 1;
  }
  {
    DpeCloudRegOptions o = opt;
    o.max_iters = 0;
    if (refused("no iterations", Q.data(), 1500, S.data(), 4000, o, "1 to 1000 iterations")) return 1;
  }
  if (refused("null source", nullptr, 1500, S.data(), 4000, opt, "bad argument")) return 1;
  if (refused("null target", Q.data(), 1500, nullptr, 4000, opt, "bad argument")) return 1;
  if (refused("2^31 sources", Q.data(), (size_t)1 << 31, S.data(), 4000, opt, "bad argument")) return 1;
  const float far2[6] = {-1e30f, 0, 0, 1e30f, 0, 0};
  opt.radius[0] = 1e-3f;
  if (refused("extent", Q.data(), 1500, far2, 2, opt, "radius too small")) return 1;
  opt.radius[0] = 0.15f;
  DpeCloudReg again;
  if (dpe_host_cloud_register(Q.data(), 1500, S.data(), 4000, &opt, -1, &again) != 0 || std::memcmp(again.T, reg.T, sizeof reg.T) != 0 ||
      again.iters[0] != reg.iters[0] || again.converged[0] != 2)
    return fail("the library is not usable after the refusals");
  std::printf("register sanitize ok\n");
  return 0;
}
