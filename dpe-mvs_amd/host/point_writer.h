// point_writer.h — the host half of the per-image point clouds of the resident runner (point_cloud = 1 / 2).
#pragma once
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host.h"

namespace dpe_host {

// submit() runs one image's point cloud on the context's stream (dpe_state_point_cloud: the colours go
// up, the kernels run, the count comes back) and starts the copy of the points into one of two pinned
// buffers sized to the full-resolution level; it blocks only while both are in flight.  The worker
// thread waits for a buffer's copy (dpe_state_point_cloud_wait), encodes and writes the PLY
// (export_point_cloud) and hands the buffer back.  finish() joins it and reports the first error.
class PointCloudWriter {
 public:
  PointCloudWriter(DpeContext* ctx, int max_w, int max_h);
  ~PointCloudWriter() { std::string e; finish(e); }
  PointCloudWriter(const PointCloudWriter&) = delete;
  PointCloudWriter& operator=(const PointCloudWriter&) = delete;

  // `cam` and `bgr` at the size of image_id's state; `bgr` may be released on return
  bool submit(int image_id, int mode, const DpeCamera& cam, const uint8_t* bgr, float dmin, float dmax,
              const std::string& path, std::string& err);
  bool finish(std::string& err);

 private:
  static constexpr int kBuffers = 2;
  struct Job { int buf; size_t n; std::string path; };
  void work();
  DpeContext* ctx_;
  std::vector<std::vector<FusedPoint>> bufs_;
  std::vector<bool> pinned_;
  std::deque<int> free_;
  std::deque<Job> jobs_;
  std::mutex mu_;
  std::condition_variable cv_free_, cv_job_;
  std::thread worker_;
  bool stop_ = false;
  std::string err_;
};

}  // namespace dpe_host
