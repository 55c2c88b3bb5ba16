// map_eval.h — what the depth-map and the normal-map evaluation share on the host, over a metric of
// csrc/depth_eval.h or csrc/normal_eval.h (DepthMetric, NormalMetric): the z-buffer of a view, the score of one map
// with the pairwise tree taken literally, total += s, the shares every score derives, and the evaluation of a dense
// folder over either path.  host/depth_eval.cpp and host/normal_eval.cpp give the metric's own parts.
#pragma once
#include "host.h"
#include "pairwise_tree.h"
#include "parallel.h"
#include "../csrc/depth_eval.h"

#include <algorithm>
#include <cstring>
#include <filesystem>
#include <string>
#include <vector>

namespace dpe_host {

constexpr size_t kRenderPerThread = 1u << 16;   // fewer points than this per thread are not worth a z-buffer

// points [i0, i1) into the z-buffer zb of dpe::RenderWord<Word>'s words
template <typename Word>
void render_range(const float* xyz, size_t i0, size_t i1, const DpeCamera& cam, int s, Word* zb) {
  const int w = cam.width, h = cam.height;
  for (size_t i = i0; i < i1; ++i) {
    int cx, cy;
    uint32_t z;
    if (!dpe::depth_point(cam, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, z)) continue;
    const Word word = dpe::RenderWord<Word>::make(z, (uint32_t)i);
    const int x0 = std::max(0, cx - s), x1 = std::min(w - 1, cx + s);
    const int y0 = std::max(0, cy - s), y1 = std::min(h - 1, cy + s);
    for (int y = y0; y <= y1; ++y) {
      Word* row = zb + (size_t)y * (size_t)w;
      for (int x = x0; x <= x1; ++x)
        if (word < row[x]) row[x] = word;
    }
  }
}

// the z-buffer of the view, one word per pixel: one buffer per thread over its share of the points, merged by minimum
template <typename Word>
std::vector<Word> render_zbuffer(const float* xyz, size_t n, const DpeCamera& cam, int splat) {
  const size_t npx = (size_t)cam.width * (size_t)cam.height;
  const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)host_threads(), n / kRenderPerThread));
  std::vector<Word> zb((size_t)nt * npx, dpe::RenderWord<Word>::kEmpty);
  run_on_threads(nt, [&](int t) { render_range(xyz, n * t / nt, n * (t + 1) / nt, cam, splat, zb.data() + (size_t)t * npx); });
  for (int t = 1; t < nt; ++t)
    for (size_t p = 0; p < npx; ++p) zb[p] = std::min(zb[p], zb[(size_t)t * npx + p]);
  zb.resize(npx);
  return zb;
}

// the score of one map against another, both checked by the caller
template <typename M>
void map_score(const float* est, const float* gt, int w, int h, const typename M::Taus& T, typename M::Score* out, float* errmap) {
  const size_t npx = (size_t)w * (size_t)h;
  float E[M::kBins + 1];
  if constexpr (M::kBins > 0) M::edges(E);
  unsigned long long counts[M::kCounters] = {};
  PairwiseTree<M::kTerms> tree;
  for (size_t i = 0; i < npx; ++i) {
    const float* e = est + M::kChannels * i;
    const float* g = gt + M::kChannels * i;
    const typename M::Pixel p = M::pixel(e, g);
    counts[0] += p.gt_ok;
    counts[1] += p.est_ok;
    counts[2] += p.both;
    for (int k = 0; k < T.n; ++k) counts[3 + k] += M::hit(p, g, T, k);
    if constexpr (M::kBins > 0) {
      if (p.both) counts[3 + M::kMaxTau + M::bin(E, p)] += 1;
    }
    double t[M::kTerms];
    M::terms(p, t);
    tree.push(t);
    if (errmap) errmap[i] = M::error_code(p);
  }
  double sums[M::kTerms];
  tree.finish(sums);
  *out = dpe::score_of<M>(npx, T.n, counts, sums);
}

template <typename M>
void score_add(typename M::Score* total, const typename M::Score& s) {
  total->n_px += s.n_px;
  total->n_gt += s.n_gt;
  total->n_est += s.n_est;
  total->n_both += s.n_both;
  for (int k = 0; k < M::kMaxTau; ++k) total->within[k] += s.within[k];
  M::add(*total, s);
}

// the head of every score's stats: within[k] / n_both and within[k] / n_gt, 0 where the divisor is
template <typename M>
void stats_shares(const typename M::Score& s, int n_tau, double* of_both, double* of_gt) {
  const double nb = (double)s.n_both, ng = (double)s.n_gt;
  for (int k = 0; k < n_tau && k < M::kMaxTau; ++k) {
    of_both[k] = s.n_both ? (double)s.within[k] / nb : 0.0;
    of_gt[k] = s.n_gt ? (double)s.within[k] / ng : 0.0;
  }
}

inline const char* map_name_or(const char* name, const char* otherwise) { return name && *name ? name : otherwise; }

// a dpe_host_read_npy_* entry over its reader: the size always, the values when `data` is given and has the room
template <typename Reader>
int read_npy_entry(Reader read, const char* path, float* data, size_t cap, int* w, int* h) {
  std::string err = "read_npy: bad argument";
  std::vector<float> v;
  int mw = 0, mh = 0;
  if (path && w && h && read(path, v, mw, mh, err)) {
    *w = mw;
    *h = mh;
    if (!data) return 0;
    if (cap >= v.size()) { std::memcpy(data, v.data(), v.size() * sizeof(float)); return 0; }
    err = "read_npy: room for fewer values than the file holds";
  }
  set_last_error(err);
  return 1;
}

// The evaluation of a dense folder: every image DPE/<id> that holds the map, in ascending id, against ground-truth
// maps or against the scan rendered into its view, on the device (o.gpu_index >= 0) or on the host.  A failure leaves
// the caller's rows and total alone.  The hooks H give the metric's own parts:
//   Metric, Options, Image; kWho (leads the messages), kMap (the default map name), kGtName / kErrName (--maps files)
//   read               the .npy reader of a map
//   args_ok            the checks of the thresholds and, for a scan, of what renders it, with their own messages
//   prepare            once per folder, for a scan: what the views need (staging; the scan's normals)
//   render_device / render_host, score_device / score_host   the four calls of one image
template <typename H>
bool map_eval(H& hk, const typename H::Options& o, const float* gt_xyz, size_t n_gt, typename H::Image* rows, size_t cap,
              size_t* n_rows, typename H::Metric::Score* total, std::string& err) {
  namespace fs = std::filesystem;
  using M = typename H::Metric;
  const std::string who = H::kWho;
  if (!o.dense_folder || !n_rows || !total || (!rows && cap)) { err = who + ": bad argument"; return false; }
  const bool from_maps = o.gt_maps_dir && *o.gt_maps_dir;
  if (!hk.args_ok(o, gt_xyz, n_gt, from_maps, err)) return false;
  const std::string dense = o.dense_folder, map = map_name_or(o.map_name, H::kMap);
  std::vector<int> ids;
  if (!eval_list(H::kWho, dense, map, ids, err)) return false;
  *n_rows = ids.size();
  if (cap < ids.size()) { err = who + ": room for fewer rows than images"; return false; }
  OwnedContext own(o.gpu_index, H::kWho, err);
  if (!own.ok) return false;
  DpeContext* ctx = own.ctx;
  auto device_failed = [&]() { err = who + ": " + dpe_last_error(); return false; };
  if (!from_maps && !hk.prepare(ctx, o, gt_xyz, n_gt, err)) return ctx ? device_failed() : false;
  typename M::Score sum;
  std::memset(&sum, 0, sizeof sum);
  std::vector<float> est, gt, errmap;
  std::vector<typename H::Image> done(ids.size());   // a failure leaves the caller's rows alone
  for (size_t i = 0; i < ids.size(); ++i) {
    const fs::path rf = fs::path(dense) / "DPE" / fmt_index(ids[i]);
    int w = 0, h = 0;
    if (!H::read((rf / map).string(), est, w, h, err)) return false;
    const size_t npx = (size_t)w * (size_t)h;
    const bool want_gt = !ctx || from_maps || o.write_maps;   // the ground truth on the host
    if (want_gt) gt.resize(M::kChannels * npx);
    if (o.write_maps) errmap.resize(npx);
    if (from_maps) {
      int gw = 0, gh = 0;
      const std::string path = (fs::path(o.gt_maps_dir) / (fmt_index(ids[i]) + ".npy")).string();
      if (!H::read(path, gt, gw, gh, err)) return false;
      if (gw != w || gh != h) { err = who + ": size mismatch: " + path + " is not of the size of " + (rf / map).string(); return false; }
    } else {
      DpeCamera cam;
      if (!map_camera(dense, ids[i], w, h, cam, err)) return false;
      if (ctx) {
        if (hk.render_device(ctx, cam, o, want_gt ? gt.data() : nullptr) != 0) return device_failed();
      } else if (!hk.render_host(gt_xyz, n_gt, cam, o, gt.data(), err)) {
        return false;
      }
    }
    typename H::Image row;
    std::memset(&row, 0, sizeof row);
    row.id = ids[i];
    row.width = w;
    row.height = h;
    float* em = o.write_maps ? errmap.data() : nullptr;
    if (ctx) {
      if (hk.score_device(ctx, est.data(), from_maps ? gt.data() : nullptr, w, h, o, &row.score, em) != 0) return device_failed();
    } else if (!hk.score_host(est.data(), gt.data(), w, h, o, &row.score, em, err)) {
      return false;
    }
    if (o.write_maps) {
      const std::vector<int64_t> hw = {h, w};
      std::vector<int64_t> shape = hw;
      if (M::kChannels > 1) shape.push_back(M::kChannels);
      if (!write_npy((rf / H::kGtName).string(), gt.data(), shape, "<f4", 4, err) ||
          !write_npy((rf / H::kErrName).string(), errmap.data(), hw, "<f4", 4, err))
        return false;
    }
    done[i] = row;
    score_add<M>(&sum, row.score);
  }
  std::copy(done.begin(), done.end(), rows);
  *total = sum;
  return true;
}

}  // namespace dpe_host
