// Drives the host normal-map evaluation (host/normal_eval.cpp over csrc/normal_eval.h, the 3-D .npy reader of
// host/hostio.cpp, the grid of host/cloud_eval.cpp, the folder helpers of host/depth_eval.cpp) under ASan + UBSan
// (tests/test_normal_eval.py): the point normals at n = 0 to 4 100 out of and into exactly sized heap buffers, their
// counts and ten sums compared with an all-pairs loop written here; the render with winners against the plain render
// and a winner loop written here; the score at 1 to 65 537 pixels against a literal pairwise tree; good and bad 3-D
// .npy files; the folder tool on a folder this program writes; and every refusal.  Linked with those sources,
// host/ply_read.cpp and host/jpeg.cpp only: the few symbols of the other libraries they refer to are defined here (no
// device path in this program).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include <unistd.h>

#include "no_device.h"

namespace fs = std::filesystem;

// ---- what host/points.cpp provides in the library, and the device entries of these sources (no_device.h: the rest)
namespace dpe_host {
void scale_intrinsics(DpeCamera& cam, float sx, float sy) { cam.K[0] *= sx; cam.K[2] *= sx; cam.K[4] *= sy; cam.K[5] *= sy; }
}  // namespace dpe_host
extern "C" int dpe_cloud_nn_pair(DpeContext*, const float*, size_t, const float*, size_t, float, float*, float*) { return DPE_ERR_ARG; }
extern "C" int dpe_cloud_render_stage(DpeContext*, const float*, size_t) { return DPE_ERR_ARG; }
extern "C" int dpe_cloud_render_view(DpeContext*, const DpeCamera*, int, float*) { return DPE_ERR_ARG; }
extern "C" int dpe_depth_score(DpeContext*, const float*, const float*, int, int, const float*, int, int, DpeDepthScore*, float*) {
  return DPE_ERR_ARG;
}
extern "C" int dpe_cloud_normals(DpeContext*, const float*, size_t, float, int, float*, int32_t*, long long*) { return DPE_ERR_ARG; }
extern "C" int dpe_cloud_render_stage_normals(DpeContext*, const float*, const float*, size_t) { return DPE_ERR_ARG; }
extern "C" int dpe_cloud_render_view_normals(DpeContext*, const DpeCamera*, int, float*, float*) { return DPE_ERR_ARG; }
extern "C" int dpe_normal_score(DpeContext*, const float*, const float*, int, int, const float*, int, DpeNormalScore*, float*) {
  return DPE_ERR_ARG;
}

static int fail(const std::string& what) {
  std::fprintf(stderr, "normal sanitize: %s (last error: %s)\n", what.c_str(), g_msg.c_str());
  return 1;
}

static unsigned g_seed = 20261021u;
static double rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (double)(g_seed >> 8) / 16777216.0; }

static uint32_t bits_of(float v) { uint32_t u; std::memcpy(&u, &v, sizeof u); return u; }
static bool usable(float v) { const uint32_t u = bits_of(v); return u > 0u && u < 0x7F800000u; }
static bool finite_bits(float v) { return (bits_of(v) & 0x7F800000u) != 0x7F800000u; }
static bool finite3(const float* p) { return finite_bits(p[0]) && finite_bits(p[1]) && finite_bits(p[2]); }

// ---- 1. point normals: counts and sums against all pairs
// kind 0: uniform in a cube of edge `spread`; kind 1: clusters of 10 within 0.8 R of centres spread over the cube, so
// that the occupied cells outnumber the buckets and neighbours sit in several cells; kind 2: a tilted plane patch at
// offset 1000
static std::vector<float> cloud_of(size_t n, int kind, float R, float spread) {
  std::vector<float> p(3 * n);
  float centre[3] = {0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    if (kind == 1 && i % 10 == 0) for (float& c : centre) c = (float)(rnd() * spread);
    for (int a = 0; a < 3; ++a) {
      if (kind == 0) p[3 * i + a] = (float)(rnd() * spread);
      else if (kind == 1) p[3 * i + a] = centre[a] + (float)((rnd() - 0.5) * 0.9 * R);
    }
    if (kind == 2) {
      const float u = (float)(i % 16) * 0.01f, v = (float)(i / 16) * 0.01f;
      p[3 * i] = 1000.f + u; p[3 * i + 1] = -1000.f + v; p[3 * i + 2] = 1000.f + 0.5f * u - 0.25f * v;
    }
  }
  if (kind == 0 && n >= 64) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    p[3 * 11] = nan; p[3 * 13 + 1] = inf; p[3 * 17 + 2] = -inf;
  }
  return p;
}

static int run_normals(size_t n, int kind, float R, float spread, int min_nb) {
  const std::vector<float> cloud = cloud_of(n, kind, R, spread);
  float* src = new float[3 * n];              // exactly sized: a read past the end is a report
  if (n) std::memcpy(src, cloud.data(), 3 * n * sizeof(float));
  float* normal = new float[3 * n];
  int32_t* count = new int32_t[n];
  long long* sums = new long long[10 * n];
  if (dpe_host_cloud_normals(src, n, R, min_nb, normal, count, sums) != 0) return fail("normals refused");
  const float R2 = R * R;
  const double S = 32768.0 / (double)R;
  size_t with_normal = 0;
  for (size_t i = 0; i < n; ++i) {
    long long want[10] = {0};
    const float* q = src + 3 * i;
    for (size_t j = 0; finite3(q) && j < n; ++j) {
      const float* t = src + 3 * j;
      if (!finite3(t)) continue;
      const float dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
      float s = dx * dx;
      s = s + dy * dy;
      s = s + dz * dz;
      if (!(s < R2)) continue;
      const long long k[3] = {(long long)((double)dx * S), (long long)((double)dy * S), (long long)((double)dz * S)};
      want[0] += 1;
      want[1] += k[0]; want[2] += k[1]; want[3] += k[2];
      want[4] += k[0] * k[0]; want[5] += k[0] * k[1]; want[6] += k[0] * k[2];
      want[7] += k[1] * k[1]; want[8] += k[1] * k[2]; want[9] += k[2] * k[2];
    }
    if (std::memcmp(want, sums + 10 * i, sizeof want) != 0 || count[i] != (int32_t)want[0])
      return fail("sums differ at point " + std::to_string(i) + " of " + std::to_string(n) + ", kind " + std::to_string(kind));
    const float* v = normal + 3 * i;
    const double len = std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
    if (len != 0.0 && std::fabs(len - 1.0) > 1e-6) return fail("a normal is neither zero nor unit");
    if (len != 0.0 && count[i] < min_nb) return fail("a normal below the neighbour count");
    if (len != 0.0) {
      ++with_normal;
      const double big = std::fmax(std::fabs(v[0]), std::fmax(std::fabs(v[1]), std::fabs(v[2])));
      if (!(v[0] == big || v[1] == big || v[2] == big)) return fail("the largest component is not positive");
    }
    if (kind == 2 && len != 0.0) {   // the patch's plane: z = 0.5 x - 0.25 y, normal (-0.5, 0.25, 1) / |.|
      const double pn[3] = {-0.5 / 1.1456439237389600, 0.25 / 1.1456439237389600, 1.0 / 1.1456439237389600};
      const double dot = std::fabs(v[0] * pn[0] + v[1] * pn[1] + v[2] * pn[2]);
      if (dot < 0.999) return fail("the patch's normal is off its plane's");   // within 2.6 degrees: the lattice at offset 1000
    }
  }
  if (kind == 2 && with_normal != n) return fail("a point of the patch has no normal");
  if (n <= 2 && with_normal != 0) return fail("a normal from fewer than 3 points");
  delete[] sums;
  delete[] count;
  delete[] normal;
  delete[] src;
  return 0;
}

// ---- 2. the render with winners
static DpeCamera pixel_camera(int w, int h) {
  DpeCamera cam;
  std::memset(&cam, 0, sizeof cam);
  cam.K[0] = cam.K[4] = cam.K[8] = 1.f;
  cam.R[0] = cam.R[4] = cam.R[8] = 1.f;
  cam.width = w;
  cam.height = h;
  return cam;
}

static int run_render(int w, int h, int s, size_t n) {
  const DpeCamera cam = pixel_camera(w, h);
  float* pts = new float[3 * n];
  float* nrm = new float[3 * n];
  const float depths[4] = {1.f, 2.f, 2.f, 4.f};
  for (size_t i = 0; i < n; ++i) {
    const float z = depths[(int)(rnd() * 4) & 3];
    pts[3 * i] = (float)std::floor(rnd() * (w + 4) - 2) * z;
    pts[3 * i + 1] = (float)std::floor(rnd() * (h + 4) - 2) * z;
    pts[3 * i + 2] = z;
    const int kind = (int)(rnd() * 4) & 3;
    nrm[3 * i] = kind == 0 ? 0.f : (float)(rnd() - 0.5);
    nrm[3 * i + 1] = kind == 0 ? 0.f : (float)(rnd() - 0.5);
    nrm[3 * i + 2] = kind == 0 ? 0.f : (kind == 1 ? 1.f : -1.f);
  }
  const size_t npx = (size_t)w * h;
  float* depth = new float[npx];
  float* plain = new float[npx];
  float* normal = new float[3 * npx];
  if (dpe_host_cloud_render_normals(pts, nrm, n, &cam, s, depth, normal) != 0) return fail("render refused");
  if (dpe_host_cloud_render(pts, n, &cam, s, plain) != 0 || std::memcmp(depth, plain, npx * sizeof(float)) != 0)
    return fail("the depth map is not the plain render's");
  // the winner per pixel, again: the lowest (z, index) among the points that cover it (identity camera: px = x / z)
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      long long best = -1;
      for (size_t i = 0; i < n; ++i) {
        const float z = pts[3 * i + 2], fx = pts[3 * i] / z + 0.5f, fy = pts[3 * i + 1] / z + 0.5f;
        if (!(fx > -1.0f && fx < (float)w && fy > -1.0f && fy < (float)h)) continue;
        const int cx = (int)fx, cy = (int)fy;
        if (std::abs(cx - x) > s || std::abs(cy - y) > s) continue;
        if (best < 0 || z < pts[3 * best + 2]) best = (long long)i;
      }
      const float* got = normal + 3 * ((size_t)y * w + x);
      float want[3] = {0.f, 0.f, 0.f};
      if (best >= 0) {
        const float* v = nrm + 3 * best;
        const float* p = pts + 3 * best;
        const float d = (v[0] * p[0] + v[1] * p[1]) + v[2] * p[2];
        const bool none = v[0] == 0.f && v[1] == 0.f && v[2] == 0.f;
        for (int a = 0; a < 3; ++a) want[a] = none ? 0.f : (d > 0.f ? -v[a] : v[a]);
      }
      if (std::memcmp(got, want, sizeof want) != 0) return fail("a pixel's normal is not its winner's");
    }
  // either output may be left out
  if (dpe_host_cloud_render_normals(pts, nrm, n, &cam, s, nullptr, normal) != 0 || dpe_host_cloud_render_normals(pts, nrm, n, &cam, s, depth, nullptr) != 0)
    return fail("an output could not be left out");
  delete[] normal;
  delete[] plain;
  delete[] depth;
  delete[] nrm;
  delete[] pts;
  return 0;
}

// ---- 3. the score
static double literal_tree(std::vector<double> s) {
  size_t n = s.size();
  while (n > 1) {
    const size_t half = (n + 1) / 2;
    for (size_t k = 0; k < half; ++k) s[k] = s[2 * k] + (2 * k + 1 < n ? s[2 * k + 1] : 0.0);
    n = half;
  }
  return n ? s[0] : 0.0;
}

static int run_score(size_t npx, bool all_invalid) {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float bad[5] = {0.f, -0.f, inf, nan, 1e20f};
  float* est = new float[3 * npx];
  float* gt = new float[3 * npx];
  float* err = new float[npx];
  for (size_t i = 0; i < npx; ++i) {
    for (int a = 0; a < 3; ++a) {
      gt[3 * i + a] = (float)(rnd() - 0.5);
      est[3 * i + a] = gt[3 * i + a] + (float)((rnd() - 0.5) * 0.3);
    }
    float* victim = all_invalid ? (i & 1 ? est : gt) : (i % 11 == 3 ? est : i % 11 == 7 ? gt : nullptr);
    if (victim) {
      const float v = bad[i % 5];
      victim[3 * i] = v;
      victim[3 * i + 1] = v == 0.f ? v : victim[3 * i + 1];
      victim[3 * i + 2] = v == 0.f ? v : victim[3 * i + 2];
    }
    if (!all_invalid && i % 11 == 9) for (int a = 0; a < 3; ++a) est[3 * i + a] = gt[3 * i + a];   // the same vector: c is 1 or a float off it
  }
  const float cos_tau[3] = {dpe_host_normal_cos(11.25), dpe_host_normal_cos(30.0), -1.0f};
  DpeNormalScore got;
  if (dpe_host_normal_score(est, gt, (int)npx, 1, cos_tau, 3, &got, err) != 0) return fail("score refused");
  float E[DPE_NORMAL_BINS];
  dpe_host_normal_edges(E);
  DpeNormalScore want;
  std::memset(&want, 0, sizeof want);
  std::vector<double> a(npx), q(npx);
  for (size_t i = 0; i < npx; ++i) {
    const float* e = est + 3 * i;
    const float* g = gt + 3 * i;
    const float ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    const bool e_ok = finite3(e) && usable(ee), g_ok = finite3(g) && usable(gg), both = e_ok && g_ok && usable(ee * gg);
    float c = ((e[0] * g[0] + e[1] * g[1]) + e[2] * g[2]) / std::sqrt(ee * gg);
    c = c < -1.f ? -1.f : (c > 1.f ? 1.f : c);
    want.n_gt += g_ok; want.n_est += e_ok; want.n_both += both;
    for (int k = 0; k < 3; ++k) want.within[k] += both && c > cos_tau[k];
    int bin = 0;
    for (int b = 1; b < DPE_NORMAL_BINS; ++b) bin += c < E[b];
    if (both) want.hist[bin] += 1;
    const double d = 1.0 - (double)c;
    a[i] = both ? d : 0.0; q[i] = both ? d * d : 0.0;
    const float code = both ? c : (g_ok ? -2.f : -3.f);
    if (bits_of(code) != bits_of(err[i])) return fail("error map differs");
  }
  want.n_px = (long long)npx;
  want.sum_dist = literal_tree(a); want.sum_dist_sq = literal_tree(q);
  if (std::memcmp(&got, &want, sizeof got) != 0) return fail("score differs at " + std::to_string(npx) + " pixels");
  long long in_hist = 0;
  for (long long v : got.hist) in_hist += v;
  if (in_hist != got.n_both) return fail("the histogram does not hold the `both` pixels");
  if (all_invalid && (got.n_both != 0 || std::signbit(got.sum_dist) || got.sum_dist != 0.0 || std::signbit(got.sum_dist_sq)))
    return fail("an invalid image does not sum to +0.0");
  DpeNormalStats st;
  dpe_host_normal_stats(&got, 3, &st);
  if (all_invalid ? (st.mean_deg != 0.0 || st.median_deg != 0.0)
                  : !(st.mean_cos_dist >= 0.0 && st.mean_deg > 0.0 && st.median_deg > 0.0 && st.share[0] <= st.share[1] && st.share[2] <= 1.0 &&
                      st.completeness[1] <= st.share[1]))
    return fail("stats");
  delete[] err;
  delete[] gt;
  delete[] est;
  return 0;
}

// ---- 4. the 3-D reader and the folder tool
static void write_npy_raw(const std::string& path, const std::string& descr, const std::string& order, const std::string& shape,
                          const void* body, size_t bytes, int major = 1) {
  std::string head = "{'descr': " + descr + ", 'fortran_order': " + order + ", 'shape': " + shape + ", }";
  head.append((16 - (10 + head.size() + 1) % 16) % 16, ' ');
  head.push_back('\n');
  std::ofstream f(path, std::ios::binary);
  f.write("\x93NUMPY", 6);
  f.put((char)major); f.put(0);
  const unsigned short hl = (unsigned short)head.size();
  f.write(reinterpret_cast<const char*>(&hl), 2);
  f.write(head.data(), (std::streamsize)head.size());
  f.write(reinterpret_cast<const char*>(body), (std::streamsize)bytes);
}

static int run_npy(const fs::path& dir) {
  const std::string p = (dir / "x.npy").string();
  float six[6] = {0.f, 1.f, 2.f, 3.f, 4.f, 5.f};
  int w = 0, h = 0;
  write_npy_raw(p, "'<f4'", "False", "(2, 1, 3)", six, sizeof six);
  float* out = new float[6];
  if (dpe_host_read_npy_f32x3(p.c_str(), nullptr, 0, &w, &h) != 0 || w != 1 || h != 2) return fail("npy size");
  if (dpe_host_read_npy_f32x3(p.c_str(), out, 6, &w, &h) != 0 || std::memcmp(out, six, sizeof six) != 0) return fail("npy data");
  if (dpe_host_read_npy_f32x3(p.c_str(), out, 5, &w, &h) == 0) return fail("npy into too small a buffer accepted");
  if (dpe_host_read_npy_f32(p.c_str(), nullptr, 0, &w, &h) == 0 || g_msg.find("2-D") == std::string::npos) return fail("the 2-D reader took a 3-D file");
  delete[] out;
  struct Bad { const char *descr, *order, *shape; size_t bytes; int major; const char* message; };
  const Bad bad[] = {{"'<f8'", "False", "(2, 1, 3)", 24, 1, "dtype"},   {"'<f4'", "True", "(2, 1, 3)", 24, 1, "Fortran"},
                     {"'<f4'", "False", "(2, 1, 3)", 23, 1, "truncated"}, {"'<f4'", "False", "(2, 1, 3)", 25, 1, "longer"},
                     {"'<f4'", "False", "(2, 3)", 24, 1, "3-D"},          {"'<f4'", "False", "(1, 3, 2)", 24, 1, "3-D"},
                     {"'<f4'", "False", "(1, 2, 3, 1)", 24, 1, "3-D"},    {"'<f4'", "False", "(0, 2, 3)", 0, 1, "3-D"},
                     {"'<f4'", "False", "(2147483647, 2147483647, 3)", 24, 1, "truncated"}, {"'<f4'", "False", "(2, 1, 3)", 24, 2, "version"}};
  const unsigned char zeros[32] = {0};
  for (const Bad& b : bad) {
    write_npy_raw(p, b.descr, b.order, b.shape, zeros, b.bytes, b.major);
    if (dpe_host_read_npy_f32x3(p.c_str(), nullptr, 0, &w, &h) == 0 || g_msg.find(b.message) == std::string::npos)
      return fail(std::string("a bad .npy accepted or misreported: ") + b.message);
  }
  if (dpe_host_read_npy_f32x3((dir / "none.npy").string().c_str(), nullptr, 0, &w, &h) == 0) return fail("a missing file accepted");
  return 0;
}

// a dense folder of two 16 x 12 views of the plane z = 4 seen from the origin, the second map at half the image's size
static int run_folder(const fs::path& dir) {
  const fs::path dense = dir / "dense";
  fs::create_directories(dense / "cams");
  fs::create_directories(dense / "images");
  fs::create_directories(dir / "gtmaps");
  const int W = 16, H = 12;
  for (int id = 0; id < 2; ++id) {
    char name[16];
    std::snprintf(name, sizeof name, "%08d", id);
    { std::ofstream f(dense / "cams" / (std::string(name) + "_cam.txt"));
      f << "extrinsic\n1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n\nintrinsic\n16 0 8\n0 16 6\n0 0 1\n\n1 0.1 64 9\n"; }
    { std::ofstream f(dense / "images" / (std::string(name) + ".jpg"), std::ios::binary);   // a binary PGM: the reader goes by content
      f << "P5\n" << W << " " << H << "\n255\n";
      const std::string px((size_t)W * H, '\x40');
      f.write(px.data(), (std::streamsize)px.size()); }
    const int w = id ? W / 2 : W, h = id ? H / 2 : H;
    std::vector<float> est((size_t)3 * w * h, 0.f);
    for (size_t p = 0; p < (size_t)w * h; ++p) est[3 * p + 2] = -1.f;      // the plane faces the camera
    est[2] = 0.f;                                                          // pixel 0: no estimate
    est[3] = 1.f; est[5] = 0.f;                                            // pixel 1: 90 degrees off
    const std::string shape = "(" + std::to_string(h) + ", " + std::to_string(w) + ", 3)";
    fs::create_directories(dense / "DPE" / name);
    write_npy_raw((dense / "DPE" / name / "normal.npy").string(), "'<f4'", "False", shape, est.data(), est.size() * 4);
    std::vector<float> gt((size_t)3 * w * h, 0.f);
    for (size_t p = 0; p < (size_t)w * h; ++p) gt[3 * p + 2] = -1.f;
    write_npy_raw((dir / "gtmaps" / (std::string(name) + ".npy")).string(), "'<f4'", "False", shape, gt.data(), gt.size() * 4);
  }
  fs::create_directories(dense / "DPE" / "00000005");   // no map: not an image
  const size_t n = (size_t)W * H;
  float* scan = new float[3 * n];                       // one point per pixel centre of the full-size view at depth 4
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      float* p = scan + 3 * ((size_t)y * W + x);
      p[0] = (float)((x - 8) / 16.0 * 4.0); p[1] = (float)((y - 6) / 16.0 * 4.0); p[2] = 4.f;
    }
  const std::string d = dense.string(), maps = (dir / "gtmaps").string();
  DpeNormalEvalOptions o;
  std::memset(&o, 0, sizeof o);
  o.dense_folder = d.c_str();
  o.radius = 0.6f;                                      // the grid's spacing is 0.25: a point's 3 x 3 neighbours and more
  o.min_nb = 3;
  o.n_tau = 2;
  o.cos_tau[0] = dpe_host_normal_cos(5.0);
  o.cos_tau[1] = dpe_host_normal_cos(120.0);
  o.gpu_index = -1;
  o.write_maps = 1;
  DpeNormalImage* rows = new DpeNormalImage[2];
  DpeNormalScore total;
  size_t k = 0;
  if (dpe_host_normal_eval(&o, scan, n, rows, 2, &k, &total) != 0 || k != 2) return fail("folder refused");
  // view 0: every pixel has a ground-truth normal (0, 0, -1); one estimate is missing, one is 90 degrees off
  if (rows[0].score.n_gt != W * H || rows[0].score.n_both != W * H - 1 || rows[0].score.within[0] != W * H - 2 ||
      rows[0].score.within[1] != W * H - 1 || rows[0].score.sum_dist != 1.0 || rows[0].score.hist[0] != W * H - 2 || rows[0].score.hist[89] + rows[0].score.hist[90] != 1)
    return fail("view 0 scored wrongly");
  if (rows[1].width != W / 2 || rows[1].score.n_gt != W * H / 4 || rows[1].score.n_both != W * H / 4 - 1) return fail("view 1 scored wrongly");
  if (total.n_px != W * H + W * H / 4 || total.sum_dist != 2.0 || total.within[0] != rows[0].score.within[0] + rows[1].score.within[0]) return fail("total");
  int w = 0, h = 0;
  float* em = new float[(size_t)W * H];
  if (dpe_host_read_npy_f32((dense / "DPE" / "00000000" / "normal_error.npy").string().c_str(), em, (size_t)W * H, &w, &h) != 0 || w != W ||
      em[0] != -2.0f || em[1] != 0.0f || em[2] != 1.0f)
    return fail("the error map was not written as scored");
  delete[] em;
  float* gm = new float[(size_t)3 * W * H];
  if (dpe_host_read_npy_f32x3((dense / "DPE" / "00000000" / "normal_gt.npy").string().c_str(), gm, (size_t)3 * W * H, &w, &h) != 0 || h != H ||
      gm[0] != 0.f || gm[2] != -1.f)
    return fail("the ground-truth map was not written as rendered");
  delete[] gm;
  // ground-truth maps instead of the scan
  DpeNormalScore total2;
  o.write_maps = 0;
  o.gt_maps_dir = maps.c_str();
  if (dpe_host_normal_eval(&o, nullptr, 0, rows, 2, &k, &total2) != 0 || total2.n_both != total.n_both || total2.sum_dist != 2.0) return fail("gt maps");
  // refusals; each must leave the rows alone
  const DpeNormalImage before = rows[0];
  auto refused = [&](const char* message) {
    const bool r = dpe_host_normal_eval(&o, scan, n, rows, 2, &k, &total2) != 0 && g_msg.find(message) != std::string::npos &&
                   std::memcmp(&before, &rows[0], sizeof before) == 0;
    if (!r) std::fprintf(stderr, "normal sanitize: expected a refusal with '%s', got '%s'\n", message, g_msg.c_str());
    return r;
  };
  write_npy_raw((dir / "gtmaps" / "00000001.npy").string(), "'<f4'", "False", "(1, 3, 3)", rows, 36);
  if (!refused("size mismatch")) return 1;
  fs::remove(dir / "gtmaps" / "00000001.npy");
  if (!refused("cannot read npy")) return 1;
  o.gt_maps_dir = nullptr;
  o.splat = 9;
  if (!refused("splat")) return 1;
  o.splat = 0;
  o.min_nb = 2;
  if (!refused("at least 3 neighbours")) return 1;
  o.min_nb = 3;
  o.radius = 0.f;
  if (!refused("radius")) return 1;
  o.radius = 0.6f;
  o.n_tau = 17;
  if (!refused("1 to 16 thresholds")) return 1;
  o.n_tau = 1;
  o.cos_tau[0] = 1.5f;
  if (!refused("not in [-1, 1]")) return 1;
  o.cos_tau[0] = 0.5f;
  if (dpe_host_normal_eval(&o, scan, n, rows, 1, &k, &total2) == 0 || k != 2) return fail("too few rows accepted");
  o.gpu_index = 0;
  if (!refused("no device in this program")) return 1;
  o.gpu_index = -1;
  fs::remove(dense / "images" / "00000001.jpg");
  if (!refused("cannot read image")) return 1;
  const std::string nowhere = (dir / "nowhere").string();
  o.dense_folder = nowhere.c_str();
  if (!refused("no DPE folder")) return 1;
  delete[] rows;
  delete[] scan;
  return 0;
}

int main() {
  for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)65, (size_t)257})
    if (run_normals(n, 0, 0.3f, 1.0f, 3)) return 1;
  if (run_normals(4100, 1, 0.02f, 1.0f, 5)) return 1;     // more occupied cells than buckets: a bucket walked twice would show
  if (run_normals(256, 2, 0.035f, 0.f, 6)) return 1;      // the plane patch at offset 1000
  if (run_normals(3000, 0, 1.0f, 0.2f, 3)) return 1;      // one cell: every point a neighbour of every point
  {
    float pt[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f}, out[9];
    int32_t cnt[3];
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (dpe_host_cloud_normals(pt, 3, 0.f, 3, out, cnt, nullptr) == 0 || dpe_host_cloud_normals(pt, 3, nan, 3, out, cnt, nullptr) == 0 ||
        dpe_host_cloud_normals(pt, 3, 2.f, 2, out, cnt, nullptr) == 0 || dpe_host_cloud_normals(nullptr, 3, 2.f, 3, out, cnt, nullptr) == 0 ||
        dpe_host_cloud_normals(pt, 3, 2.f, 3, nullptr, cnt, nullptr) == 0 || dpe_host_cloud_normals(pt, 3, 2.f, 3, out, nullptr, nullptr) == 0 ||
        dpe_host_cloud_normals(pt, (size_t)1 << 31, 2.f, 3, out, cnt, nullptr) == 0)
      return fail("bad normals accepted");
    if (dpe_host_cloud_normals(pt, 3, 2.f, 3, out, cnt, nullptr) != 0 || cnt[0] != 3 || out[2] != 1.f || out[8] != 1.f) return fail("three points in a plane");
  }
  const int sizes[3][2] = {{1, 1}, {7, 5}, {65, 33}};
  for (const auto& wh : sizes)
    for (int s : {0, 1, 2})
      for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)1000})
        if (run_render(wh[0], wh[1], s, n)) return 1;
  if (run_render(7, 5, 0, 200000)) return 1;   // enough points for several host threads
  {
    DpeCamera cam = pixel_camera(7, 5);
    float px[35], nm[105], pt[3] = {0.f, 0.f, 1.f};
    if (dpe_host_cloud_render_normals(pt, pt, 1, &cam, 9, px, nm) == 0 || dpe_host_cloud_render_normals(pt, nullptr, 1, &cam, 0, px, nm) == 0 ||
        dpe_host_cloud_render_normals(nullptr, pt, 1, &cam, 0, px, nm) == 0 || dpe_host_cloud_render_normals(pt, pt, 1, nullptr, 0, px, nm) == 0)
      return fail("a bad render accepted");
    cam.width = 0;
    if (dpe_host_cloud_render_normals(pt, pt, 1, &cam, 0, px, nm) == 0) return fail("an empty camera accepted");
  }
  const size_t pixels[5] = {1, 255, 256, 257, 65537};
  for (size_t npx : pixels)
    for (int invalid = 0; invalid < 2; ++invalid)
      if (run_score(npx, invalid != 0)) return 1;
  {
    float one[3] = {1.f, 0.f, 0.f}, tau = 0.5f, nan = std::numeric_limits<float>::quiet_NaN(), big = 1.5f;
    DpeNormalScore s;
    if (dpe_host_normal_score(one, one, 1, 1, &tau, 0, &s, nullptr) == 0 || dpe_host_normal_score(one, one, 1, 1, &tau, 17, &s, nullptr) == 0 ||
        dpe_host_normal_score(one, one, 0, 1, &tau, 1, &s, nullptr) == 0 || dpe_host_normal_score(one, nullptr, 1, 1, &tau, 1, &s, nullptr) == 0 ||
        dpe_host_normal_score(one, one, 1, 1, &nan, 1, &s, nullptr) == 0 || dpe_host_normal_score(one, one, 1, 1, &big, 1, &s, nullptr) == 0 ||
        dpe_host_normal_score(one, one, 1, 1, &tau, 1, nullptr, nullptr) == 0)
      return fail("a bad score accepted");
  }
  std::error_code ec;
  const fs::path dir = fs::temp_directory_path() / ("normal_sanitize_" + std::to_string((unsigned long long)std::hash<std::string>{}(std::to_string(g_seed)) ^ (unsigned long long)::getpid()));
  fs::remove_all(dir, ec);
  fs::create_directories(dir);
  const int rc = run_npy(dir) || run_folder(dir);
  fs::remove_all(dir, ec);
  if (rc) return 1;
  std::printf("normal sanitize ok\n");
  return 0;
}
