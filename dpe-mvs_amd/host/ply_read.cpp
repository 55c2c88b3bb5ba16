// ply_read.cpp — reads the points of a PLY file (dpe_host_read_point_cloud): `ascii` and
// `binary_little_endian 1.0`, the `vertex` element's scalar properties x, y, z (float or double, at any
// position; a double is rounded to float), every other scalar property skipped by its size, elements after
// `vertex` ignored.  It reads what export_point_cloud (fusion.cpp) writes.  The file comes from outside: every
// count and size is checked before it is used, and nothing is trusted beyond the bytes that were read.
// dpe_host_read_point_cloud_rgb also returns the three uchar colours such a file carries (diffuse_blue / green /
// red, or blue / green / red), as (b, g, r), and says whether the file had them.
#include "host.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

namespace dpe_host {
namespace {

struct FileCloser { void operator()(FILE* f) const { if (f) std::fclose(f); } };

// bytes of a PLY scalar type, 0 for an unknown name
int ply_type_size(const std::string& t) {
  if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
  if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
  if (t == "int" || t == "uint" || t == "int32" || t == "uint32" || t == "float" || t == "float32") return 4;
  if (t == "double" || t == "float64") return 8;
  return 0;
}
bool ply_is_float(const std::string& t) { return t == "float" || t == "float32"; }
bool ply_is_double(const std::string& t) { return t == "double" || t == "float64"; }

struct PlyProperty { std::string type, name; int size = 0; bool list = false; };
struct PlyElement { std::string name; unsigned long long count = 0; std::vector<PlyProperty> props; };

// one header line without its line end; false at the end of the file or for a line of 1 KiB or more
bool header_line(FILE* f, std::string& line) {
  char buf[1024];
  if (!std::fgets(buf, sizeof buf, f)) return false;
  size_t n = std::strlen(buf);
  if (n == 0 || buf[n - 1] != '\n') { if (n + 1 >= sizeof buf) return false; }
  while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) --n;
  line.assign(buf, n);
  return true;
}

// a decimal count that fits 2^31 - 1 (the limit of a cloud here)
bool parse_count(const std::string& s, unsigned long long& v) {
  if (s.empty() || s.size() > 19) return false;
  v = 0;
  for (char ch : s) {
    if (ch < '0' || ch > '9') return false;
    v = v * 10 + (unsigned long long)(ch - '0');
  }
  return true;
}

}  // namespace

// the reader behind read_point_cloud and read_point_cloud_rgb: rgb / has_rgb null for the positions alone
static bool read_ply_vertices(const std::string& path, float* xyz, uint8_t* rgb, size_t cap, size_t* n, int* has_rgb,
                              std::string& err) {
  if (!n) { err = "read_point_cloud: null argument"; return false; }
  *n = 0;
  if (has_rgb) *has_rgb = 0;
  std::unique_ptr<FILE, FileCloser> file(std::fopen(path.c_str(), "rb"));
  FILE* f = file.get();
  if (!f) { err = "cannot read " + path; return false; }
  std::string line;
  if (!header_line(f, line) || line != "ply") { err = path + ": not a PLY file"; return false; }
  bool binary = false, have_format = false, ended = false;
  std::vector<PlyElement> elems;
  while (header_line(f, line)) {
    std::istringstream in(line);
    std::string key;
    in >> key;
    if (key == "end_header") { ended = true; break; }
    if (key.empty() || key == "comment" || key == "obj_info") continue;
    if (key == "format") {
      std::string fmt, ver;
      in >> fmt >> ver;
      if (fmt == "binary_big_endian") { err = path + ": big-endian PLY files are not supported"; return false; }
      if ((fmt != "ascii" && fmt != "binary_little_endian") || ver != "1.0") { err = path + ": unknown PLY format"; return false; }
      binary = fmt == "binary_little_endian";
      have_format = true;
    } else if (key == "element") {
      PlyElement e;
      std::string cnt;
      in >> e.name >> cnt;
      if (e.name.empty() || !parse_count(cnt, e.count) || e.count > (unsigned long long)INT_MAX) {
        err = path + ": the count of element '" + e.name + "' does not fit";
        return false;
      }
      elems.push_back(e);
    } else if (key == "property") {
      if (elems.empty()) { err = path + ": property before any element"; return false; }
      PlyProperty p;
      in >> p.type;
      if (p.type == "list") {
        std::string ct, it;
        in >> ct >> it >> p.name;
        p.list = true;
      } else {
        in >> p.name;
        p.size = ply_type_size(p.type);
        if (p.size == 0 || p.name.empty()) { err = path + ": unknown property type '" + p.type + "'"; return false; }
      }
      elems.back().props.push_back(p);
    } else {
      err = path + ": unknown header line '" + key + "'";
      return false;
    }
  }
  if (!ended || !have_format) { err = path + ": truncated PLY header"; return false; }
  size_t vi = 0;
  while (vi < elems.size() && elems[vi].name != "vertex") ++vi;
  if (vi == elems.size()) { err = path + ": no vertex element"; return false; }
  const PlyElement& V = elems[vi];
  // where x, y, z sit in a vertex
  int col[3] = {-1, -1, -1}, off[3] = {0, 0, 0};
  bool dbl[3] = {false, false, false};
  // and the three uchar colours of a PLY of ours, in the order blue, green, red
  static const char* const kColour[3][2] = {{"diffuse_blue", "blue"}, {"diffuse_green", "green"}, {"diffuse_red", "red"}};
  int ccol[3] = {-1, -1, -1}, coff[3] = {0, 0, 0};
  size_t stride = 0;
  for (size_t k = 0; k < V.props.size(); ++k) {
    const PlyProperty& p = V.props[k];
    if (p.list) { err = path + ": a list property inside the vertex element is not supported"; return false; }
    for (int a = 0; a < 3; ++a) {
      if (ccol[a] >= 0 || (p.type != "uchar" && p.type != "uint8") || (p.name != kColour[a][0] && p.name != kColour[a][1])) continue;
      ccol[a] = (int)k; coff[a] = (int)stride;
    }
    for (int a = 0; a < 3; ++a) {
      if (p.name != std::string(1, "xyz"[a]) || col[a] >= 0) continue;
      if (!ply_is_float(p.type) && !ply_is_double(p.type)) { err = path + ": coordinate " + p.name + " is neither float nor double"; return false; }
      col[a] = (int)k; off[a] = (int)stride; dbl[a] = ply_is_double(p.type);
    }
    stride += (size_t)p.size;
  }
  for (int a = 0; a < 3; ++a)
    if (col[a] < 0) { err = path + ": missing coordinate " + std::string(1, "xyz"[a]); return false; }
  // the elements in front of the vertices are skipped: scalar properties only
  for (size_t e = 0; e < vi; ++e) {
    size_t sz = 0;
    for (const PlyProperty& p : elems[e].props) {
      if (p.list) { err = path + ": a list property in front of the vertex element is not supported"; return false; }
      sz += (size_t)p.size;
    }
    if (binary) {
      const unsigned long long bytes = (unsigned long long)sz * elems[e].count;
      if (bytes > (unsigned long long)LONG_MAX || std::fseek(f, (long)bytes, SEEK_CUR) != 0) { err = path + ": truncated body"; return false; }
    } else {
      for (unsigned long long k = 0; k < elems[e].count; ++k)
        if (!header_line(f, line)) { err = path + ": truncated body"; return false; }
    }
  }
  *n = (size_t)V.count;
  const bool colours = ccol[0] >= 0 && ccol[1] >= 0 && ccol[2] >= 0;
  if (has_rgb) *has_rgb = colours ? 1 : 0;
  if (!xyz) return true;   // size query
  if (!colours) rgb = nullptr;
  if (cap < *n) { err = path + ": point buffer too small"; return false; }
  if (binary) {
    const size_t kBatch = 4096;
    std::vector<unsigned char> buf(kBatch * stride);
    for (size_t i0 = 0; i0 < *n; i0 += kBatch) {
      const size_t k = std::min(kBatch, *n - i0);
      if (std::fread(buf.data(), stride, k, f) != k) { err = path + ": truncated body"; return false; }
      for (size_t i = 0; i < k; ++i) {
        const unsigned char* v = buf.data() + i * stride;
        for (int a = 0; a < 3; ++a) {
          if (dbl[a]) { double d; std::memcpy(&d, v + off[a], 8); xyz[3 * (i0 + i) + a] = (float)d; }
          else std::memcpy(&xyz[3 * (i0 + i) + a], v + off[a], 4);
          if (rgb) rgb[3 * (i0 + i) + a] = v[coff[a]];
        }
      }
    }
    return true;
  }
  // ascii: one vertex per line, its properties separated by blanks
  std::vector<char> text;
  for (size_t i = 0; i < *n; ++i) {
    text.clear();
    int ch;
    while ((ch = std::fgetc(f)) != EOF && ch != '\n') text.push_back((char)ch);
    if (ch == EOF && text.empty()) { err = path + ": truncated body"; return false; }
    text.push_back('\0');
    const char* p = text.data();
    for (int k = 0; k < (int)V.props.size(); ++k) {
      char* end = nullptr;
      const double d = std::strtod(p, &end);
      if (end == p) { err = path + ": truncated body"; return false; }
      for (int a = 0; a < 3; ++a)
        if (col[a] == k) xyz[3 * i + a] = dbl[a] ? (float)d : std::strtof(p, nullptr);
      for (int a = 0; a < 3; ++a)
        if (rgb && ccol[a] == k) rgb[3 * i + a] = (uint8_t)(d >= 255.0 ? 255 : d > 0.0 ? (int)d : 0);
      p = end;
    }
  }
  return true;
}

bool read_point_cloud(const std::string& path, float* xyz, size_t cap, size_t* n, std::string& err) {
  return read_ply_vertices(path, xyz, nullptr, cap, n, nullptr, err);
}

bool read_point_cloud_rgb(const std::string& path, float* xyz, uint8_t* rgb, size_t cap, size_t* n, int* has_rgb,
                          std::string& err) {
  return read_ply_vertices(path, xyz, rgb, cap, n, has_rgb, err);
}

}  // namespace dpe_host

extern "C" int dpe_host_read_point_cloud_rgb(const char* path, float* xyz, uint8_t* rgb, size_t cap, size_t* n, int* has_rgb) {
  std::string err;
  if (path && dpe_host::read_point_cloud_rgb(path, xyz, rgb, cap, n, has_rgb, err)) return 0;
  dpe_host::set_last_error(path ? err : "read_point_cloud: null argument");
  return 1;
}

extern "C" int dpe_host_read_point_cloud(const char* path, float* xyz, size_t cap, size_t* n) {
  std::string err;
  if (path && dpe_host::read_point_cloud(path, xyz, cap, n, err)) return 0;
  dpe_host::set_last_error(path ? err : "read_point_cloud: null argument");
  return 1;
}
