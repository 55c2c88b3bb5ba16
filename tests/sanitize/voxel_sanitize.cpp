// Drives the host voxel down-sampling and the crop (host/cloud_voxel.cpp) and the colour reader
// (host/ply_read.cpp) under ASan + UBSan (tests/test_cloud_voxel.py).  The host loop runs on an adversarial cloud
// (offsets of +-1000, points on voxel faces and an ulp to either side), on 1 000 copies of one point and on
// non-finite points, into heap buffers of exactly the size it is given, and is compared with a serial check of the
// records' set properties; the reader gets good and malformed files from memory-backed files (memfd).  Linked with
// those two sources only: the few symbols of the other libraries they refer to are defined here (no device path
// and no distances in this program).
#include <sys/mman.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "no_device.h"

// ---- what host/cloud_eval.cpp provides in the library, and the device entry of these sources (no_device.h: the rest)
namespace dpe_host {
bool cloud_eval_in(DpeContext*, const float*, size_t, const float*, size_t, const float*, int, float, DpeCloudEval*, std::string& err) {
  err = "no distances in this program";
  return false;
}
bool cloud_eval(const float*, size_t, const float*, size_t, const float*, int, float, int, DpeCloudEval*, std::string& err) {
  err = "no distances in this program";
  return false;
}
}  // namespace dpe_host
extern "C" int dpe_cloud_voxel(DpeContext*, const float*, size_t, const uint8_t*, float, float*, uint8_t*, int32_t*, int32_t*, size_t,
                               size_t*) { return DPE_ERR_ARG; }

static int fail(const std::string& what) {
  std::fprintf(stderr, "voxel sanitize: %s (last error: %s)\n", what.c_str(), g_msg.c_str());
  return 1;
}

// a file in memory holding `bytes`; its path is /proc/self/fd/<fd>
struct MemFile {
  int fd = -1;
  std::string path;
  explicit MemFile(const std::string& bytes) {
    fd = memfd_create("voxel_sanitize", 0);
    if (fd < 0) return;
    size_t done = 0;
    while (done < bytes.size()) {
      const ssize_t k = write(fd, bytes.data() + done, bytes.size() - done);
      if (k <= 0) break;
      done += (size_t)k;
    }
    path = "/proc/self/fd/" + std::to_string(fd);
  }
  ~MemFile() { if (fd >= 0) close(fd); }
};

template <class T>
static void put(std::string& s, T v) { s.append(reinterpret_cast<const char*>(&v), sizeof v); }

// reads `bytes` with the colour reader into exactly sized heap buffers: 0, the points and colours, or 1 and the message
static int read_ply(const std::string& bytes, std::vector<float>& xyz, std::vector<uint8_t>& rgb, int& has) {
  MemFile f(bytes);
  if (f.fd < 0) { g_msg = "memfd_create failed"; return -1; }
  size_t n = 0;
  if (dpe_host_read_point_cloud_rgb(f.path.c_str(), nullptr, nullptr, 0, &n, &has) != 0) return 1;
  float* buf = new float[3 * n + 1];
  uint8_t* col = new uint8_t[3 * n + 1];
  std::memset(col, 0xAB, 3 * n + 1);
  const int rc = dpe_host_read_point_cloud_rgb(f.path.c_str(), buf, col, n, &n, &has);
  xyz.assign(buf, buf + 3 * n);
  rgb.assign(col, col + 3 * n);
  delete[] buf;
  delete[] col;
  return rc;
}

static int expect_fail(const char* name, const std::string& bytes, const char* needle) {
  std::vector<float> xyz;
  std::vector<uint8_t> rgb;
  int has = 0;
  g_msg.clear();
  const int rc = read_ply(bytes, xyz, rgb, has);
  if (rc < 0) return fail("memfd");
  if (rc == 0) return fail(std::string(name) + ": a malformed file was accepted");
  if (g_msg.find(needle) == std::string::npos) return fail(std::string(name) + ": message without '" + needle + "'");
  return 0;
}

// Runs the host loop on n points (with colours when rgb is not null) into exactly sized buffers and checks what
// holds whatever the arithmetic: ascending first, each the lowest index of a distinct cell (cells recomputed here
// in double), counts that sum to the finite points, every record inside its voxel's closed box, and the colour
// means by an independent sum.
static int run_voxel(const char* name, const std::vector<float>& P, const std::vector<uint8_t>* rgb, float v) {
  const size_t n = P.size() / 3;
  size_t k = 0;
  // first the number of voxels (cap 0 writes nothing), then buffers of exactly that size
  const int rc0 = dpe_host_cloud_voxel(P.data(), n, rgb ? rgb->data() : nullptr, v, nullptr, nullptr, nullptr, nullptr, 0, &k);
  if (k == 0) return rc0 == 0 ? 0 : fail(std::string(name) + ": refused");
  if (rc0 == 0) return fail(std::string(name) + ": cap 0 accepted");
  float* xyz = new float[3 * k];
  uint8_t* col = new uint8_t[3 * k];
  int32_t* first = new int32_t[k];
  int32_t* count = new int32_t[k];
  size_t k2 = 0;
  if (dpe_host_cloud_voxel(P.data(), n, rgb ? rgb->data() : nullptr, v, xyz, rgb ? col : nullptr, first, count, k, &k2) != 0 || k2 != k)
    return fail(std::string(name) + ": second call");
  double o[3] = {0, 0, 0};
  bool any = false;
  size_t finite = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* p = &P[3 * i];
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
    for (int a = 0; a < 3; ++a) if (!any || (double)p[a] < o[a]) o[a] = (double)p[a];
    any = true;
    ++finite;
  }
  typedef std::tuple<long long, long long, long long> Key;
  std::map<Key, size_t> seen;                 // cell -> record, in the order of meeting
  std::vector<size_t> low, cnt;
  std::vector<unsigned long long> csum;
  for (size_t i = 0; i < n; ++i) {
    const float* p = &P[3 * i];
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
    long long c[3];
    for (int a = 0; a < 3; ++a) c[a] = (long long)std::floor(((double)p[a] - o[a]) / (double)v);
    const auto it = seen.emplace(Key(c[0], c[1], c[2]), low.size());
    if (it.second) { low.push_back(i); cnt.push_back(0); csum.insert(csum.end(), 3, 0ull); }
    const size_t r = it.first->second;
    ++cnt[r];
    if (rgb) for (int a = 0; a < 3; ++a) csum[3 * r + a] += (*rgb)[3 * i + a];
  }
  if (low.size() != k) return fail(std::string(name) + ": number of voxels");
  size_t total = 0;
  for (size_t r = 0; r < k; ++r) {
    if ((size_t)first[r] != low[r] || (size_t)count[r] != cnt[r]) return fail(std::string(name) + ": first / count of record " + std::to_string(r));
    total += (size_t)count[r];
    const float* p = &P[3 * low[r]];
    for (int a = 0; a < 3; ++a) {
      const double c = std::floor(((double)p[a] - o[a]) / (double)v);
      const double lo = o[a] + c * (double)v, hi = o[a] + (c + 1.0) * (double)v;
      const double slack = std::fabs(hi) * 0x1p-22 + (double)v * 0x1p-20;   // the float rounding of the record
      if (!((double)xyz[3 * r + a] >= lo - slack && (double)xyz[3 * r + a] <= hi + slack))
        return fail(std::string(name) + ": record " + std::to_string(r) + " outside its voxel");
      if (rgb && col[3 * r + a] != (uint8_t)((2 * csum[3 * r + a] + cnt[r]) / (2 * cnt[r])))
        return fail(std::string(name) + ": colour of record " + std::to_string(r));
    }
  }
  if (total != finite) return fail(std::string(name) + ": counts");
  delete[] xyz; delete[] col; delete[] first; delete[] count;
  return 0;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  auto add = [](std::vector<float>& v, float x, float y, float z) { v.push_back(x); v.push_back(y); v.push_back(z); };
  unsigned seed = 12345u;
  auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.0f; };
  // ---- adversarial: offsets of +-1000, points on voxel faces and their float neighbours, a crowded voxel
  const float v = 0.0625f * 1.1f;
  std::vector<float> A;
  for (int i = 0; i < 300; ++i) add(A, 1000.0f + rnd(), -1000.0f + rnd(), rnd());
  for (int i = 0; i < 300; ++i) add(A, -1000.0f + rnd(), 1000.0f + rnd(), -rnd());
  for (int i = 0; i < 400; ++i) add(A, 1000.5f + 0.01f * rnd(), -999.5f + 0.01f * rnd(), 0.5f + 0.01f * rnd());
  for (int i = -3; i < 40; ++i) {
    const float x = -1000.0f + (float)i * v;
    add(A, x, 0, 0); add(A, std::nextafter(x, -inf), 0, 0); add(A, std::nextafter(x, inf), 0, 0);
  }
  std::vector<uint8_t> AC(A.size());
  for (uint8_t& c : AC) c = (uint8_t)(rnd() * 256.0f);
  if (run_voxel("adversarial", A, nullptr, v) || run_voxel("adversarial with colours", A, &AC, v) ||
      run_voxel("adversarial, 4 v", A, &AC, 4.0f * v)) return 1;
  // ---- same: 1 000 copies of one point and one other point
  std::vector<float> S;
  for (int i = 0; i < 1000; ++i) add(S, 0.3f, 1000.7f, -5.1f);
  add(S, 0.3f, 1001.7f, -5.1f);
  std::vector<uint8_t> SC(S.size(), 255);
  if (run_voxel("same", S, &SC, 0.05f)) return 1;
  // ---- non-finite points among finite ones, and nothing but them
  std::vector<float> N;
  for (int i = 0; i < 200; ++i) add(N, rnd(), rnd(), rnd());
  add(N, nan, 0, 0); add(N, 0, inf, 0); add(N, 0, 0, -inf); add(N, nan, nan, nan);
  std::swap(N[0], N[3 * 200]);   // a non-finite coordinate in the first point
  std::vector<uint8_t> NC(N.size(), 7);
  if (run_voxel("nonfinite", N, &NC, 0.25f)) return 1;
  std::vector<float> bad;
  for (int i = 0; i < 5; ++i) add(bad, nan, inf, -inf);
  size_t k = 99;
  if (dpe_host_cloud_voxel(bad.data(), 5, nullptr, 0.25f, nullptr, nullptr, nullptr, nullptr, 0, &k) != 0 || k != 0) return fail("all non-finite");
  if (dpe_host_cloud_voxel(nullptr, 0, nullptr, 0.25f, nullptr, nullptr, nullptr, nullptr, 0, &k) != 0 || k != 0) return fail("empty cloud");
  // ---- argument errors
  float one[3] = {0, 0, 0}, ox[3];
  int32_t of = 0, oc = 0;
  for (float w : {0.0f, -1.0f, nan, inf})
    if (dpe_host_cloud_voxel(one, 1, nullptr, w, ox, nullptr, &of, &oc, 1, &k) == 0 || g_msg.find("bad argument") == std::string::npos)
      return fail("bad voxel accepted");
  const float far2[6] = {-1e30f, 0, 0, 1e30f, 0, 0};
  float o2[6];
  int32_t f2[2], c2[2];
  if (dpe_host_cloud_voxel(far2, 2, nullptr, 1e-3f, o2, nullptr, f2, c2, 2, &k) == 0 || g_msg.find("voxel too small") == std::string::npos)
    return fail("extent accepted");
  if (dpe_host_cloud_voxel(one, 1, nullptr, 1.0f, ox, nullptr, &of, &oc, 1, &k) != 0 || k != 1 || of != 0 || oc != 1) return fail("one point");
  // ---- crop: both ends inclusive, NaN dropped, order kept, exactly sized outputs
  {
    const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    std::vector<float> C;
    add(C, 0, 0, 0); add(C, 1, 1, 1); add(C, nan, 0.5f, 0.5f); add(C, 2, 2, 2); add(C, 0.5f, 0.5f, 0.5f); add(C, 0.5f, inf, 0.5f);
    std::vector<uint8_t> CC(C.size());
    for (size_t i = 0; i < CC.size(); ++i) CC[i] = (uint8_t)i;
    const size_t kk = dpe_host_cloud_crop(C.data(), 6, CC.data(), lo, hi, nullptr, nullptr, nullptr);
    if (kk != 3) return fail("crop count");
    float* cx = new float[3 * kk];
    uint8_t* cc = new uint8_t[3 * kk];
    int32_t* ci = new int32_t[kk];
    if (dpe_host_cloud_crop(C.data(), 6, CC.data(), lo, hi, cx, cc, ci) != 3 || ci[0] != 0 || ci[1] != 1 || ci[2] != 4 || cx[6] != 0.5f ||
        cc[6] != 12)
      return fail("crop");
    delete[] cx; delete[] cc; delete[] ci;
  }
  // ---- the prepared evaluation reaches the (absent) distances only after a valid preparation
  {
    DpeCloudPrep prep{};
    DpeCloudEval e;
    const float tau[1] = {0.1f};
    prep.voxel = 0.25f;
    prep.use_crop = 1;
    for (int a = 0; a < 3; ++a) { prep.crop_lo[a] = 0.0f; prep.crop_hi[a] = 0.9f; }
    if (dpe_host_cloud_eval_prep(N.data(), N.size() / 3, A.data(), A.size() / 3, tau, 1, 0.0f, -1, &prep, &e) == 0 ||
        g_msg.find("no distances") == std::string::npos || prep.n_recon_in != N.size() / 3)
      return fail("prepared evaluation");
    prep.voxel = -1.0f;
    if (dpe_host_cloud_eval_prep(N.data(), N.size() / 3, A.data(), A.size() / 3, tau, 1, 0.0f, -1, &prep, &e) == 0 ||
        g_msg.find("voxel edge") == std::string::npos)
      return fail("bad voxel edge accepted");
  }
  // ---- the colour reader: good files
  const float pts[3][3] = {{1.5f, -2.25f, 3.0f}, {0.0f, 1e-3f, -7.0f}, {1000.5f, 2.0f, 0.125f}};
  std::vector<float> xyz;
  std::vector<uint8_t> rgb;
  int has = 0;
  {  // what the writer writes: float xyz + 3 uchar
    std::string s = "ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                    "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n";
    for (auto& p : pts) { put(s, p[0]); put(s, p[1]); put(s, p[2]); put(s, (unsigned char)1); put(s, (unsigned char)2); put(s, (unsigned char)3); }
    if (read_ply(s, xyz, rgb, has) != 0 || !has || xyz.size() != 9 || std::memcmp(xyz.data(), pts, sizeof pts) != 0 || rgb[0] != 1 ||
        rgb[4] != 2 || rgb[8] != 3)
      return fail("binary colour file");
    if (expect_fail("truncated binary", s.substr(0, s.size() - 2), "truncated body")) return 1;
  }
  {  // colours by their short names, scattered among doubles; an element in front and one behind
    std::string s = "ply\nformat binary_little_endian 1.0\nelement camera 2\nproperty int id\nelement vertex 3\nproperty uchar red\n"
                    "property double z\nproperty uint8 green\nproperty double x\nproperty double y\nproperty uchar blue\n"
                    "element face 1\nproperty list uchar int vertex_indices\nend_header\n";
    put(s, 7); put(s, 8);
    for (auto& p : pts) { put(s, (unsigned char)30); put(s, (double)p[2]); put(s, (unsigned char)20); put(s, (double)p[0]); put(s, (double)p[1]); put(s, (unsigned char)10); }
    if (read_ply(s, xyz, rgb, has) != 0 || !has || std::memcmp(xyz.data(), pts, sizeof pts) != 0 || rgb[0] != 10 || rgb[1] != 20 || rgb[2] != 30)
      return fail("binary named colours");
  }
  {  // ascii with colours, and a file without them (one channel is not a colour)
    const std::string head = "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty uchar blue\nproperty float y\n"
                             "property uchar green\nproperty double z\nproperty uchar red\nend_header\n";
    if (read_ply(head + "1.5 0 -2.25 128 3 255\n0 1 1e-3 2 -7 3\r\n1000.5 9 2 8 0.125 7", xyz, rgb, has) != 0 || !has ||
        std::memcmp(xyz.data(), pts, sizeof pts) != 0 || rgb[0] != 0 || rgb[1] != 128 || rgb[2] != 255 || rgb[8] != 7)
      return fail("ascii colour file");
    if (expect_fail("truncated ascii", head + "1.5 0 -2.25 128 3 255\n0 1 1e-3 2 -7\n", "truncated body")) return 1;
    const std::string plain = "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                              "property uchar red\nend_header\n1 2 3 4\n";
    if (read_ply(plain, xyz, rgb, has) != 0 || has || xyz.size() != 3 || rgb[0] != 0xAB) return fail("file without colours");
    if (read_ply("ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n", xyz, rgb, has) != 0 ||
        !xyz.empty())
      return fail("empty file");
  }
  // ---- the colour reader: malformed files, refused as by the position reader
  const std::string xyzp = "property float x\nproperty float y\nproperty float z\n";
  if (expect_fail("list", "ply\nformat ascii 1.0\nelement vertex 1\n" + xyzp + "property list uchar int n\nend_header\n0 0 0 0\n", "list property")) return 1;
  if (expect_fail("big endian", "ply\nformat binary_big_endian 1.0\nelement vertex 1\n" + xyzp + "end_header\n", "big-endian")) return 1;
  if (expect_fail("count", "ply\nformat ascii 1.0\nelement vertex 2147483648\n" + xyzp + "end_header\n", "does not fit")) return 1;
  if (expect_fail("missing z", "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n", "missing coordinate z")) return 1;
  if (expect_fail("no header end", "ply\nformat ascii 1.0\nelement vertex 1\n" + xyzp, "truncated PLY header")) return 1;
  if (expect_fail("not ply", "plx\n", "not a PLY")) return 1;
  if (expect_fail("empty", "", "not a PLY")) return 1;
  std::printf("voxel sanitize ok\n");
  return 0;
}
