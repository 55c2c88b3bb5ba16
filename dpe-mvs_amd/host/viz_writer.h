// viz_writer.h — the host half of the viz pictures of the resident runner (viz = true).
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host.h"

namespace dpe_host {

extern const char* const kVizNames[3];   // "depth_", "normal_", "weak_": DPE_VIZ_DEPTH / NORMAL / WEAK
constexpr int kVizQuality = 95;          // cv::imwrite's default

// submit() enqueues one picture's render, JPEG front half and block copy on the context's stream
// into one of a fixed set of pinned buffers (sized to the full-resolution level) and returns; it
// blocks only while every buffer is in flight.  The worker threads wait for a buffer's copy
// (dpe_state_render_wait), Huffman-code it into the file and hand the buffer back.  finish() joins
// them and reports the first error.
class VizWriter {
 public:
  VizWriter(DpeContext* ctx, int max_w, int max_h);
  ~VizWriter() { std::string e; finish(e); }
  VizWriter(const VizWriter&) = delete;
  VizWriter& operator=(const VizWriter&) = delete;

  bool submit(int image_id, int kind, float dmin, float dmax, int w, int h, const std::string& path, std::string& err);
  bool finish(std::string& err);

 private:
  static constexpr int kBuffers = 6;   // two images' three pictures
  struct Job { int buf; std::string path; int w, h; };
  void work();
  DpeContext* ctx_;
  std::vector<std::vector<int16_t>> bufs_;
  std::vector<bool> pinned_;
  std::deque<int> free_;
  std::deque<Job> jobs_;
  std::mutex mu_;
  std::condition_variable cv_free_, cv_job_;
  std::vector<std::thread> pool_;
  bool stop_ = false;
  std::string err_;
};

}  // namespace dpe_host
