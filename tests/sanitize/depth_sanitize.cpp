// Drives the host depth-map evaluation (host/depth_eval.cpp over csrc/depth_eval.h, the .npy reader of
// host/hostio.cpp, host/ply_read.cpp) under ASan + UBSan (tests/test_depth_eval.py): the render at n = 0 to 4097 into
// 1 x 1, 7 x 5 and 65 x 33 images with half-widths 0, 1, 2 and 8, out of and into exactly sized heap buffers, compared
// bit for bit with a loop written here; the score at 1 to 65 537 pixels in both modes against a literal pairwise
// tree; good and bad .npy files; the folder tool on a folder this program writes, with a scan read from a PLY and with
// ground-truth maps; and every refusal.  Linked with those sources and host/jpeg.cpp only: the few symbols of the
// other libraries they refer to are defined here (no device path in this program).
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
extern "C" int dpe_cloud_render_stage(DpeContext*, const float*, size_t) { return DPE_ERR_ARG; }
extern "C" int dpe_cloud_render_view(DpeContext*, const DpeCamera*, int, float*) { return DPE_ERR_ARG; }
extern "C" int dpe_depth_score(DpeContext*, const float*, const float*, int, int, const float*, int, int, DpeDepthScore*, float*) {
  return DPE_ERR_ARG;
}

static int fail(const std::string& what) {
  std::fprintf(stderr, "depth sanitize: %s (last error: %s)\n", what.c_str(), g_msg.c_str());
  return 1;
}

static unsigned g_seed = 20261020u;
static double rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (double)(g_seed >> 8) / 16777216.0; }

static uint32_t bits_of(float v) { uint32_t u; std::memcpy(&u, &v, sizeof u); return u; }
static bool usable(float v) { const uint32_t u = bits_of(v); return u > 0u && u < 0x7F800000u; }
static bool finite_bits(float v) { return (bits_of(v) & 0x7F800000u) != 0x7F800000u; }

// a camera that looks down a tilted axis from (off, -off, off), focal length 1.2 w
static DpeCamera tilted_camera(int w, int h, float off) {
  DpeCamera cam;
  std::memset(&cam, 0, sizeof cam);
  const float a = 0.3f, b = -0.2f;
  const float R[9] = {std::cos(b), 0.f, std::sin(b), std::sin(a) * std::sin(b), std::cos(a), -std::sin(a) * std::cos(b),
                      -std::cos(a) * std::sin(b), std::sin(a), std::cos(a) * std::cos(b)};
  const float C[3] = {off, -off, off};
  for (int k = 0; k < 9; ++k) cam.R[k] = R[k];
  for (int r = 0; r < 3; ++r) cam.t[r] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
  cam.K[0] = cam.K[4] = 1.2f * (float)w;
  cam.K[2] = (float)w / 2.f;
  cam.K[5] = (float)h / 2.f;
  cam.K[8] = 1.f;
  cam.width = w;
  cam.height = h;
  return cam;
}

// n points in front of `cam`, some off every border, on a few depths; from 64 on also points that render nothing
static std::vector<float> scan_for(const DpeCamera& cam, size_t n, float off) {
  std::vector<float> p(3 * n);
  const float depths[4] = {1.5f, 2.f, 2.f, 7.f};
  for (size_t i = 0; i < n; ++i) {
    const double px = rnd() * (cam.width + 8) - 4, py = rnd() * (cam.height + 8) - 4, z = depths[(int)(rnd() * 4) & 3];
    const double ray[3] = {(px - cam.K[2]) / cam.K[0] * z, (py - cam.K[5]) / cam.K[4] * z, z};   // in the camera's frame
    const double C[3] = {off, -off, off};
    for (int k = 0; k < 3; ++k) p[3 * i + k] = (float)(C[k] + cam.R[k] * ray[0] + cam.R[3 + k] * ray[1] + cam.R[6 + k] * ray[2]);
  }
  if (n >= 64) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int k = 0; k < 3; ++k) p[3 * 3 + k] = (k == 0 ? off : k == 1 ? -off : off) - 2.f * cam.R[6 + k];   // behind
    p[3 * 5] = off; p[3 * 5 + 1] = -off; p[3 * 5 + 2] = off;                                               // at the centre
    p[3 * 7] = p[3 * 7 + 1] = p[3 * 7 + 2] = 3e38f;                                                        // the depth overflows
    p[3 * 11] = nan; p[3 * 13 + 1] = inf; p[3 * 17 + 2] = -inf;
  }
  return p;
}

// the contract's render, written again
static void render_again(const float* p, size_t n, const DpeCamera& c, int s, std::vector<float>& out) {
  const int w = c.width, h = c.height;
  std::vector<uint32_t> zb((size_t)w * h, 0x7F800000u);
  for (size_t i = 0; i < n; ++i) {
    const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
    if (!finite_bits(x) || !finite_bits(y) || !finite_bits(z)) continue;
    const float tx = c.R[0] * x + c.R[1] * y + c.R[2] * z + c.t[0];
    const float ty = c.R[3] * x + c.R[4] * y + c.R[5] * z + c.t[1];
    const float tz = c.R[6] * x + c.R[7] * y + c.R[8] * z + c.t[2];
    const float d = c.K[6] * tx + c.K[7] * ty + c.K[8] * tz;
    if (!usable(d)) continue;
    const float fx = (c.K[0] * tx + c.K[1] * ty + c.K[2] * tz) / d + 0.5f, fy = (c.K[3] * tx + c.K[4] * ty + c.K[5] * tz) / d + 0.5f;
    if (!(fx > -1.0f && fx < (float)w && fy > -1.0f && fy < (float)h)) continue;
    const int cx = (int)fx, cy = (int)fy;
    for (int dy = -s; dy <= s; ++dy)
      for (int dx = -s; dx <= s; ++dx) {
        const int xx = cx + dx, yy = cy + dy;
        if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
        uint32_t& at = zb[(size_t)yy * w + xx];
        if (bits_of(d) < at) at = bits_of(d);
      }
  }
  out.resize(zb.size());
  for (size_t q = 0; q < zb.size(); ++q) {
    const uint32_t u = zb[q] == 0x7F800000u ? 0u : zb[q];
    std::memcpy(&out[q], &u, sizeof u);
  }
}

static int run_render(int w, int h, int s, size_t n, float off) {
  const DpeCamera cam = tilted_camera(w, h, off);
  const std::vector<float> scan = scan_for(cam, n, off);
  float* src = new float[3 * n];              // exactly sized: a read past the end is a report
  if (n) std::memcpy(src, scan.data(), 3 * n * sizeof(float));
  float* out = new float[(size_t)w * h];
  if (dpe_host_cloud_render(src, n, &cam, s, out) != 0) return fail("render refused");
  std::vector<float> want;
  render_again(src, n, cam, s, want);
  if (std::memcmp(out, want.data(), want.size() * sizeof(float)) != 0)
    return fail("render differs at " + std::to_string(w) + "x" + std::to_string(h) + " s " + std::to_string(s) + " n " + std::to_string(n));
  delete[] out;
  delete[] src;
  return 0;
}

// the contract's tree, literally: level by level over all the terms
static double literal_tree(std::vector<double> s) {
  size_t n = s.size();
  while (n > 1) {
    const size_t half = (n + 1) / 2;
    for (size_t k = 0; k < half; ++k) s[k] = s[2 * k] + (2 * k + 1 < n ? s[2 * k + 1] : 0.0);
    n = half;
  }
  return n ? s[0] : 0.0;
}

static int run_score(size_t npx, int mode, bool all_invalid) {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float bad[6] = {0.f, -0.f, -1.f, inf, -inf, nan};
  float* est = new float[npx];
  float* gt = new float[npx];
  float* err = new float[npx];
  for (size_t i = 0; i < npx; ++i) {
    gt[i] = (float)(1 + (int)(rnd() * 4));
    est[i] = gt[i] + (float)(rnd() - 0.5);
    if (all_invalid) (i & 1 ? est[i] : gt[i]) = bad[i % 6];
    else if (i % 11 == 3) est[i] = bad[(i / 11) % 6];
    else if (i % 11 == 7) gt[i] = bad[(i / 11) % 6];
    else if (i % 11 == 9) est[i] = gt[i] + 0.5f;   // e == tau: strictly not within
  }
  const float tau[4] = {0.f, 0.125f, 0.5f, 2.f};
  DpeDepthScore got;
  if (dpe_host_depth_score(est, gt, (int)npx, 1, tau, 4, mode, &got, err) != 0) return fail("score refused");
  DpeDepthScore want;
  std::memset(&want, 0, sizeof want);
  std::vector<double> a(npx), r(npx), q(npx);
  for (size_t i = 0; i < npx; ++i) {
    const bool g = usable(gt[i]), e = usable(est[i]), both = g && e;
    const float d = std::fabs(est[i] - gt[i]), rel = d / gt[i];
    want.n_gt += g; want.n_est += e; want.n_both += both;
    for (int k = 0; k < 4; ++k) want.within[k] += both && (mode == DPE_DEPTH_TAU_ABS ? d < tau[k] : d < tau[k] * gt[i]);
    a[i] = both ? (double)d : 0.0; r[i] = both ? (double)rel : 0.0; q[i] = both ? (double)d * (double)d : 0.0;
    const float code = both ? d : (g ? -1.f : -2.f);
    if (bits_of(code) != bits_of(err[i])) return fail("error map differs");
  }
  want.n_px = (long long)npx;
  want.sum_abs = literal_tree(a); want.sum_rel = literal_tree(r); want.sum_sq = literal_tree(q);
  if (std::memcmp(&got, &want, sizeof got) != 0) return fail("score differs at " + std::to_string(npx) + " pixels, mode " + std::to_string(mode));
  if (all_invalid && (got.n_both != 0 || std::signbit(got.sum_abs) || got.sum_abs != 0.0 || std::signbit(got.sum_sq))) return fail("an invalid image does not sum to +0.0");
  DpeDepthStats st;
  dpe_host_depth_stats(&got, 4, &st);
  if (all_invalid ? st.mae != 0.0 : !(st.mae > 0.0 && st.rmse >= st.mae && st.accuracy[3] <= 1.0 && st.completeness[3] <= st.accuracy[3])) return fail("stats");
  delete[] err;
  delete[] gt;
  delete[] est;
  return 0;
}

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
  write_npy_raw(p, "'<f4'", "False", "(2, 3)", six, sizeof six);
  float* out = new float[6];
  if (dpe_host_read_npy_f32(p.c_str(), nullptr, 0, &w, &h) != 0 || w != 3 || h != 2) return fail("npy size");
  if (dpe_host_read_npy_f32(p.c_str(), out, 6, &w, &h) != 0 || std::memcmp(out, six, sizeof six) != 0) return fail("npy data");
  if (dpe_host_read_npy_f32(p.c_str(), out, 5, &w, &h) == 0) return fail("npy into too small a buffer accepted");
  delete[] out;
  struct Bad { const char *descr, *order, *shape; size_t bytes; int major; const char* message; };
  const Bad bad[] = {{"'<f8'", "False", "(2, 3)", 24, 1, "dtype"},   {"'<f4'", "True", "(2, 3)", 24, 1, "Fortran"},
                     {"'<f4'", "False", "(2, 3)", 23, 1, "truncated"}, {"'<f4'", "False", "(2, 3)", 0, 1, "truncated"},
                     {"'<f4'", "False", "(6,)", 24, 1, "2-D"},         {"'<f4'", "False", "(1, 2, 3)", 24, 1, "2-D"},
                     {"'<f4'", "False", "(99999999999, 3)", 24, 1, "2-D"}, {"'<f4'", "False", "(2147483647, 2147483647)", 24, 1, "truncated"},
                     {"'<f4'", "False", "(2, 3", 24, 1, "2-D"},        {"'<f4'", "False", "(2, 3)", 24, 2, "version"}};
  const unsigned char zeros[32] = {0};
  for (const Bad& b : bad) {
    write_npy_raw(p, b.descr, b.order, b.shape, zeros, b.bytes, b.major);
    if (dpe_host_read_npy_f32(p.c_str(), nullptr, 0, &w, &h) == 0 || g_msg.find(b.message) == std::string::npos)
      return fail(std::string("a bad .npy accepted or misreported: ") + b.message);
  }
  { std::ofstream f(p, std::ios::binary); f.write("\x93NUMPY\x01\x00\xff\xff{", 11); }
  if (dpe_host_read_npy_f32(p.c_str(), nullptr, 0, &w, &h) == 0) return fail("a truncated header accepted");
  { std::ofstream f(p, std::ios::binary); f.write("\x93NU", 3); }
  if (dpe_host_read_npy_f32(p.c_str(), nullptr, 0, &w, &h) == 0) return fail("a stub accepted");
  if (dpe_host_read_npy_f32((dir / "none.npy").string().c_str(), nullptr, 0, &w, &h) == 0) return fail("a missing file accepted");
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
    std::vector<float> est((size_t)w * h, 4.0f), gt((size_t)w * h, 4.0f);
    est[0] = 4.25f;
    est[1] = 0.f;
    fs::create_directories(dense / "DPE" / name);
    write_npy_raw((dense / "DPE" / name / "depth.npy").string(), "'<f4'", "False", "(" + std::to_string(h) + ", " + std::to_string(w) + ")",
                  est.data(), est.size() * 4);
    write_npy_raw((dir / "gtmaps" / (std::string(name) + ".npy")).string(), "'<f4'", "False",
                  "(" + std::to_string(h) + ", " + std::to_string(w) + ")", gt.data(), gt.size() * 4);
  }
  fs::create_directories(dense / "DPE" / "00000005");   // no map: not an image
  // the scan: one point per pixel centre of the full-size view at depth 4, through an ascii PLY
  { std::ofstream f(dir / "gt.ply");
    f << "ply\nformat ascii 1.0\nelement vertex " << W * H << "\nproperty float x\nproperty float y\nproperty float z\nend_header\n";
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) f << (x - 8) / 16.0 * 4.0 << " " << (y - 6) / 16.0 * 4.0 << " 4\n"; }
  size_t n = 0;
  if (dpe_host_read_point_cloud((dir / "gt.ply").string().c_str(), nullptr, 0, &n) != 0 || n != (size_t)W * H) return fail("ply size");
  float* scan = new float[3 * n];
  if (dpe_host_read_point_cloud((dir / "gt.ply").string().c_str(), scan, n, &n) != 0) return fail("ply data");
  const std::string d = dense.string(), maps = (dir / "gtmaps").string();
  size_t k = 0;
  int ids[2] = {-1, -1};
  if (dpe_host_depth_eval_list(d.c_str(), nullptr, ids, 2, &k) != 0 || k != 2 || ids[0] != 0 || ids[1] != 1) return fail("list");
  DpeDepthEvalOptions o;
  std::memset(&o, 0, sizeof o);
  o.dense_folder = d.c_str();
  o.n_tau = 2;
  o.tau[0] = 0.1f;
  o.tau[1] = 0.5f;
  o.gpu_index = -1;
  o.write_maps = 1;
  DpeDepthImage* rows = new DpeDepthImage[2];
  DpeDepthScore total;
  if (dpe_host_depth_eval(&o, scan, n, rows, 2, &k, &total) != 0) return fail("folder refused");
  // view 0: every pixel covered, one estimate off by 0.25, one missing; view 1 at half size: covered as well
  if (rows[0].score.n_gt != W * H || rows[0].score.n_both != W * H - 1 || rows[0].score.within[0] != W * H - 2 ||
      rows[0].score.within[1] != W * H - 1 || rows[0].score.sum_abs != 0.25)
    return fail("view 0 scored wrongly");
  if (rows[1].width != W / 2 || rows[1].score.n_gt != W * H / 4 || rows[1].score.n_both != W * H / 4 - 1) return fail("view 1 scored wrongly");
  if (total.n_px != W * H + W * H / 4 || total.sum_abs != 0.5 || total.within[0] != rows[0].score.within[0] + rows[1].score.within[0]) return fail("total");
  int w = 0, h = 0;
  float* em = new float[(size_t)W * H];
  if (dpe_host_read_npy_f32((dense / "DPE" / "00000000" / "depth_error.npy").string().c_str(), em, (size_t)W * H, &w, &h) != 0 || w != W ||
      em[0] != 0.25f || em[1] != -1.0f || em[2] != 0.0f)
    return fail("the error map was not written as scored");
  delete[] em;
  // ground-truth maps instead of the scan
  DpeDepthScore total2;
  o.write_maps = 0;
  o.gt_maps_dir = maps.c_str();
  o.mode = DPE_DEPTH_TAU_REL;
  if (dpe_host_depth_eval(&o, nullptr, 0, rows, 2, &k, &total2) != 0 || total2.n_both != total.n_both || total2.sum_rel != 0.125) return fail("gt maps");
  // refusals; each must leave the rows alone
  const DpeDepthImage before = rows[0];
  auto refused = [&](const char* message) {
    const bool r = dpe_host_depth_eval(&o, scan, n, rows, 2, &k, &total2) != 0 && g_msg.find(message) != std::string::npos &&
                   std::memcmp(&before, &rows[0], sizeof before) == 0;
    if (!r) std::fprintf(stderr, "depth sanitize: expected a refusal with '%s', got '%s'\n", message, g_msg.c_str());
    return r;
  };
  write_npy_raw((dir / "gtmaps" / "00000001.npy").string(), "'<f4'", "False", "(3, 3)", rows, 36);
  if (!refused("size mismatch")) return 1;
  fs::remove(dir / "gtmaps" / "00000001.npy");
  if (!refused("cannot read npy")) return 1;
  o.gt_maps_dir = nullptr;
  o.map_name = "depth_none.npy";
  if (!refused("no such map")) return 1;
  o.map_name = nullptr;
  o.splat = 9;
  if (!refused("splat")) return 1;
  o.splat = 0;
  o.n_tau = 17;
  if (!refused("1 to 16 thresholds")) return 1;
  o.n_tau = 1;
  o.tau[0] = -1.f;
  if (!refused("negative or not finite")) return 1;
  o.tau[0] = 0.1f;
  o.mode = 7;
  if (!refused("mode")) return 1;
  o.mode = 0;
  if (dpe_host_depth_eval(&o, scan, n, rows, 1, &k, &total2) == 0 || k != 2) return fail("too few rows accepted");
  o.gpu_index = 0;
  if (!refused("no device in this program")) return 1;
  o.gpu_index = -1;
  fs::remove(dense / "images" / "00000001.jpg");
  if (!refused("cannot read image")) return 1;
  delete[] rows;
  delete[] scan;
  return 0;
}

int main() {
  const int sizes[3][2] = {{1, 1}, {7, 5}, {65, 33}};
  const int splats[4] = {0, 1, 2, 8};
  const size_t counts[7] = {0, 1, 63, 64, 65, 257, 4097};
  for (const auto& wh : sizes)
    for (int s : splats)
      for (size_t n : counts)
        if (run_render(wh[0], wh[1], s, n, s == 1 ? -1000.f : 1000.f)) return 1;
  if (run_render(7, 5, 0, 200000, 0.f)) return 1;   // enough points for several host threads
  // the render's refusals
  {
    DpeCamera cam = tilted_camera(7, 5, 0.f);
    float px[35], pt[3] = {0.f, 0.f, 1.f};
    if (dpe_host_cloud_render(pt, 1, &cam, 9, px) == 0 || dpe_host_cloud_render(pt, 1, &cam, -1, px) == 0 ||
        dpe_host_cloud_render(nullptr, 1, &cam, 0, px) == 0 || dpe_host_cloud_render(pt, 1, nullptr, 0, px) == 0 ||
        dpe_host_cloud_render(pt, 1, &cam, 0, nullptr) == 0 || dpe_host_cloud_render(pt, (size_t)1 << 31, &cam, 0, px) == 0)
      return fail("a bad render accepted");
    cam.width = 0;
    if (dpe_host_cloud_render(pt, 1, &cam, 0, px) == 0) return fail("an empty camera accepted");
  }
  const size_t pixels[5] = {1, 255, 256, 257, 65537};
  for (size_t npx : pixels)
    for (int mode = 0; mode < 2; ++mode)
      for (int invalid = 0; invalid < 2; ++invalid)
        if (run_score(npx, mode, invalid != 0)) return 1;
  {
    float one = 1.f, tau = 0.1f, nan = std::numeric_limits<float>::quiet_NaN();
    DpeDepthScore s;
    if (dpe_host_depth_score(&one, &one, 1, 1, &tau, 0, 0, &s, nullptr) == 0 || dpe_host_depth_score(&one, &one, 1, 1, &tau, 17, 0, &s, nullptr) == 0 ||
        dpe_host_depth_score(&one, &one, 0, 1, &tau, 1, 0, &s, nullptr) == 0 || dpe_host_depth_score(&one, nullptr, 1, 1, &tau, 1, 0, &s, nullptr) == 0 ||
        dpe_host_depth_score(&one, &one, 1, 1, &nan, 1, 0, &s, nullptr) == 0 || dpe_host_depth_score(&one, &one, 1, 1, &tau, 1, 2, &s, nullptr) == 0 ||
        dpe_host_depth_score(&one, &one, 1, 1, &tau, 1, 0, nullptr, nullptr) == 0)
      return fail("a bad score accepted");
  }
  std::error_code ec;
  const fs::path dir = fs::temp_directory_path() / ("depth_sanitize_" + std::to_string((unsigned long long)std::hash<std::string>{}(std::to_string(g_seed)) ^ (unsigned long long)::getpid()));
  fs::remove_all(dir, ec);
  fs::create_directories(dir);
  const int rc = run_npy(dir) || run_folder(dir);
  fs::remove_all(dir, ec);
  if (rc) return 1;
  std::printf("depth sanitize ok\n");
  return 0;
}
