// Drives the PLY reader (host/ply_read.cpp) and the host grid of the cloud evaluation (host/cloud_eval.cpp)
// under ASan + UBSan (tests/test_cloud_eval.py).  The reader gets good files and every malformed case from
// memory-backed temporary files (memfd) into heap buffers of exactly the size it is given; the grid runs on a
// small adversarial cloud (offsets of +-1000, queries at the radius, a crowded cell, non-finite points) and
// is compared with a brute-force loop.  Linked with those two sources only: the few symbols of the other
// libraries they refer to are defined here (no device path in this program).
#include <sys/mman.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "no_device.h"

// ---- the device entry of these sources (no_device.h: the rest of what the library provides)
extern "C" int dpe_cloud_nn_pair(DpeContext*, const float*, size_t, const float*, size_t, float, float*, float*) { return DPE_ERR_ARG; }

static int fail(const std::string& what) {
  std::fprintf(stderr, "cloud sanitize: %s (last error: %s)\n", what.c_str(), g_msg.c_str());
  return 1;
}

// a file in memory holding `bytes`; its path is /proc/self/fd/<fd>
struct MemFile {
  int fd = -1;
  std::string path;
  explicit MemFile(const std::string& bytes) {
    fd = memfd_create("cloud_sanitize", 0);
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

// reads `bytes` as a PLY into an exactly sized heap buffer: 0 and the points, or 1 and the message
static int read_ply(const std::string& bytes, std::vector<float>& xyz) {
  MemFile f(bytes);
  if (f.fd < 0) { g_msg = "memfd_create failed"; return -1; }
  size_t n = 0;
  if (dpe_host_read_point_cloud(f.path.c_str(), nullptr, 0, &n) != 0) return 1;
  float* buf = new float[3 * n + 1];   // + 1: never a zero-sized array
  const int rc = dpe_host_read_point_cloud(f.path.c_str(), buf, n, &n);
  xyz.assign(buf, buf + 3 * n);
  delete[] buf;
  return rc;
}

static int expect_fail(const char* name, const std::string& bytes, const char* needle) {
  std::vector<float> xyz;
  g_msg.clear();
  const int rc = read_ply(bytes, xyz);
  if (rc < 0) return fail("memfd");
  if (rc == 0) return fail(std::string(name) + ": a malformed file was accepted");
  if (g_msg.find(needle) == std::string::npos) return fail(std::string(name) + ": message without '" + needle + "'");
  return 0;
}

static float brute(const float* q, const std::vector<float>& t, float radius) {
  float best = radius * radius;
  if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]))) return best;
  for (size_t j = 0; j + 2 < t.size(); j += 3) {
    if (!(std::isfinite(t[j]) && std::isfinite(t[j + 1]) && std::isfinite(t[j + 2]))) continue;
    const float dx = q[0] - t[j], dy = q[1] - t[j + 1], dz = q[2] - t[j + 2];
    float s = dx * dx;
    s = s + dy * dy;
    s = s + dz * dz;
    best = s < best ? s : best;
  }
  return best;
}

int main() {
  // ---- the reader: good files
  const float pts[3][3] = {{1.5f, -2.25f, 3.0f}, {0.0f, 1e-3f, -7.0f}, {1000.5f, 2.0f, 0.125f}};
  std::vector<float> xyz;
  {  // what the writer writes: float xyz + 3 uchar
    std::string s = "ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                    "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n";
    for (auto& p : pts) { put(s, p[0]); put(s, p[1]); put(s, p[2]); put(s, (unsigned char)1); put(s, (unsigned char)2); put(s, (unsigned char)3); }
    if (read_ply(s, xyz) != 0 || xyz.size() != 9 || std::memcmp(xyz.data(), pts, sizeof pts) != 0) return fail("binary float file");
    if (expect_fail("truncated binary", s.substr(0, s.size() - 5), "truncated body")) return 1;
  }
  {  // double coordinates behind other properties, an element in front and one behind
    std::string s = "ply\nformat binary_little_endian 1.0\ncomment made by hand\nelement camera 2\nproperty int id\n"
                    "element vertex 3\nproperty uchar red\nproperty short q\nproperty double z\nproperty double x\nproperty int k\n"
                    "property double y\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n";
    put(s, 7); put(s, 8);
    for (auto& p : pts) { put(s, (unsigned char)9); put(s, (short)-3); put(s, (double)p[2]); put(s, (double)p[0]); put(s, 11); put(s, (double)p[1]); }
    put(s, (unsigned char)3); put(s, 0); put(s, 1); put(s, 2);
    if (read_ply(s, xyz) != 0 || xyz.size() != 9 || std::memcmp(xyz.data(), pts, sizeof pts) != 0) return fail("binary double file");
  }
  {  // ascii
    const std::string head = "ply\nformat ascii 1.0\nelement vertex 3\nproperty uchar a\nproperty float x\nproperty float y\nproperty double z\nend_header\n";
    const std::string body = "5 1.5 -2.25 3\n6 0 1e-3 -7\r\n7 1000.5 2 0.125";
    if (read_ply(head + body, xyz) != 0 || xyz.size() != 9 || std::memcmp(xyz.data(), pts, sizeof pts) != 0) return fail("ascii file");
    if (expect_fail("truncated ascii", head + "5 1.5 -2.25 3\n6 0 1e-3\n", "truncated body")) return 1;
    if (expect_fail("short ascii", head + "5 1.5 -2.25 3\n", "truncated body")) return 1;
  }
  {  // an empty cloud
    if (read_ply("ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n", xyz) != 0 ||
        !xyz.empty())
      return fail("empty file");
  }
  // ---- the reader: malformed files
  const std::string xyzp = "property float x\nproperty float y\nproperty float z\n";
  if (expect_fail("list", "ply\nformat ascii 1.0\nelement vertex 1\n" + xyzp + "property list uchar int n\nend_header\n0 0 0 0\n", "list property")) return 1;
  if (expect_fail("big endian", "ply\nformat binary_big_endian 1.0\nelement vertex 1\n" + xyzp + "end_header\n", "big-endian")) return 1;
  if (expect_fail("count", "ply\nformat ascii 1.0\nelement vertex 2147483648\n" + xyzp + "end_header\n", "does not fit")) return 1;
  if (expect_fail("long count", "ply\nformat ascii 1.0\nelement vertex 99999999999999999999999\n" + xyzp + "end_header\n", "does not fit")) return 1;
  if (expect_fail("negative count", "ply\nformat ascii 1.0\nelement vertex -1\n" + xyzp + "end_header\n", "does not fit")) return 1;
  if (expect_fail("missing z", "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n", "missing coordinate z")) return 1;
  if (expect_fail("int x", "ply\nformat ascii 1.0\nelement vertex 1\nproperty int x\nproperty float y\nproperty float z\nend_header\n0 0 0\n", "neither float nor double")) return 1;
  if (expect_fail("no header end", "ply\nformat ascii 1.0\nelement vertex 1\n" + xyzp, "truncated PLY header")) return 1;
  if (expect_fail("not ply", "plx\n", "not a PLY")) return 1;
  if (expect_fail("empty", "", "not a PLY")) return 1;
  if (expect_fail("long line", "ply\ncomment " + std::string(5000, 'x') + "\n", "truncated PLY header")) return 1;
  if (expect_fail("no vertex", "ply\nformat ascii 1.0\nelement face 0\nend_header\n", "no vertex element")) return 1;
  if (expect_fail("bad type", "ply\nformat ascii 1.0\nelement vertex 1\nproperty quad x\nend_header\n", "unknown property type")) return 1;

  // ---- the host grid against brute force on a small adversarial cloud
  const float R = 0.05f, inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> T, Q;
  auto add = [](std::vector<float>& v, float x, float y, float z) { v.push_back(x); v.push_back(y); v.push_back(z); };
  unsigned seed = 12345u;
  auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.0f; };
  for (int i = 0; i < 300; ++i) add(T, 1000.0f + rnd(), -1000.0f + rnd(), rnd());
  for (int i = 0; i < 400; ++i) add(T, 1000.5f + 0.01f * rnd(), -999.5f + 0.01f * rnd(), 0.5f + 0.01f * rnd());   // a crowded cell
  add(T, nan, 0, 0); add(T, 0, inf, 0); add(T, 0, 0, -inf);
  const size_t m = T.size() / 3;
  for (size_t j = 0; j < 300; ++j) {   // at the radius from a target, along axes and diagonals, an ulp or so inside
    const float* t = &T[3 * j];
    const int k = (int)(j % 4), d = (int)(j % 26);
    const int u[3] = {d % 3 - 1, (d / 3) % 3 - 1, d / 9 - 1 + (d == 13 ? 1 : 0)};
    const float len = std::sqrt((float)(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]));
    const float r = R * (1.0f - (float)(k == 3 ? 64 : k) * 0x1p-24f) / len;
    add(Q, t[0] + r * (float)u[0], t[1] + r * (float)u[1], t[2] + r * (float)u[2]);
  }
  for (int i = 0; i < 200; ++i) add(Q, 999.9f + 1.2f * rnd(), -1000.1f + 1.2f * rnd(), -0.1f + 1.2f * rnd());
  for (int i = -3; i < 25; ++i) add(Q, 1000.0f + (float)i * R, -1000.0f + (float)i * R * (1.0f + 0x1p-23f), (float)i * R * (1.0f - 0x1p-23f));
  add(Q, nan, 1, 1); add(Q, 1, -inf, 1); add(Q, 3e38f, -3e38f, 3e38f); add(Q, -1e30f, 0, 0);
  const size_t n = Q.size() / 3;
  float* out = new float[n];
  if (dpe_host_cloud_nn(Q.data(), n, T.data(), m, R, out) != 0) return fail("cloud_nn");
  for (size_t i = 0; i < n; ++i) {
    const float b = brute(&Q[3 * i], T, R);
    if (std::memcmp(&b, &out[i], 4) != 0) return fail("cloud_nn differs from brute force at query " + std::to_string(i));
  }
  delete[] out;
  // degenerate sizes, the evaluation and its argument errors
  float one[3] = {0, 0, 0}, d = -1.0f;
  if (dpe_host_cloud_nn(one, 1, nullptr, 0, R, &d) != 0 || d != R * R) return fail("empty target");
  if (dpe_host_cloud_nn(nullptr, 0, one, 1, R, nullptr) != 0) return fail("empty query");
  if (dpe_host_cloud_nn(one, 1, one, 1, 0.0f, &d) == 0 || dpe_host_cloud_nn(one, 1, one, 1, nan, &d) == 0) return fail("bad radius accepted");
  const float far2[6] = {-1e30f, 0, 0, 1e30f, 0, 0};
  if (dpe_host_cloud_nn(one, 1, far2, 2, 1e-3f, &d) == 0 || g_msg.find("radius too small") == std::string::npos) return fail("extent accepted");
  DpeCloudEval e;
  const float tau[2] = {0.01f, 0.05f};
  if (dpe_host_cloud_eval(Q.data(), n, T.data(), m, tau, 2, 0.0f, -1, &e) == 0) return fail("extent accepted as a target");
  const size_t ne = n - 2;   // without the two far points, which no grid of this radius spans
  if (dpe_host_cloud_eval(Q.data(), ne, T.data(), m, tau, 2, 0.0f, -1, &e) != 0 || e.n_tau != 2 || e.radius != 0.05f ||
      e.dropped_recon != 2 || e.dropped_gt != 3 || !(e.fscore[0] <= e.fscore[1]))
    return fail("cloud_eval");
  float many[17];
  for (float& t : many) t = 0.01f;
  if (dpe_host_cloud_eval(Q.data(), ne, T.data(), m, many, 17, 0.0f, -1, &e) == 0) return fail("17 thresholds accepted");
  if (dpe_host_cloud_eval(Q.data(), ne, T.data(), m, tau, 2, 0.02f, -1, &e) == 0) return fail("tau above the radius accepted");
  if (dpe_host_cloud_eval(Q.data(), ne, T.data(), m, tau, 2, 0.0f, 0, &e) == 0) return fail("a device in this program");
  std::printf("cloud sanitize ok\n");
  return 0;
}
