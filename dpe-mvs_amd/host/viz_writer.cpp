// viz_writer.cpp — see viz_writer.h.
#include "viz_writer.h"

#include <algorithm>

#include "parallel.h"

namespace dpe_host {

const char* const kVizNames[3] = {"depth_", "normal_", "weak_"};

VizWriter::VizWriter(DpeContext* ctx, int max_w, int max_h) : ctx_(ctx) {
  const size_t values = jpeg_block_count(max_w, max_h, 3) * 64;
  bufs_.resize(kBuffers);
  for (int i = 0; i < kBuffers; ++i) {
    bufs_[i].resize(values);
    pinned_.push_back(dpe_host_pin(bufs_[i].data(), values * sizeof(int16_t)) == 0);   // refused: pageable, still works
    free_.push_back(i);
  }
  const int nt = std::max(1, std::min(host_threads(), kBuffers));
  for (int t = 0; t < nt; ++t) pool_.emplace_back([this]() { work(); });
}

bool VizWriter::submit(int image_id, int kind, float dmin, float dmax, int w, int h, const std::string& path,
                       std::string& err) {
  int b;
  {
    std::unique_lock<std::mutex> lk(mu_);
    cv_free_.wait(lk, [this]() { return !free_.empty(); });
    b = free_.front(); free_.pop_front();
  }
  const int rc = dpe_state_render_jpeg_blocks(ctx_, image_id, kind, dmin, dmax, kVizQuality, bufs_[b].data(), bufs_[b].size(), nullptr);
  std::lock_guard<std::mutex> lk(mu_);
  if (rc != 0) {
    err = std::string("viz render failed: ") + dpe_last_error();
    free_.push_back(b);
    return false;
  }
  jobs_.push_back(Job{b, path, w, h});
  cv_job_.notify_one();
  return true;
}

bool VizWriter::finish(std::string& err) {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_job_.notify_all();
  for (auto& th : pool_) th.join();
  pool_.clear();
  for (size_t i = 0; i < bufs_.size(); ++i)
    if (pinned_[i]) { dpe_host_unpin(bufs_[i].data()); pinned_[i] = false; }
  err = err_;
  return err_.empty();
}

void VizWriter::work() {
  for (;;) {
    Job j;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_job_.wait(lk, [this]() { return stop_ || !jobs_.empty(); });
      if (jobs_.empty()) return;
      j = std::move(jobs_.front()); jobs_.pop_front();
    }
    std::string e;
    bool ok = dpe_state_render_wait(ctx_, bufs_[j.buf].data()) == 0;
    if (!ok) e = std::string("viz render failed: ") + dpe_last_error();
    else ok = jpeg_write_blocks(j.path, bufs_[j.buf].data(), j.w, j.h, 3, kVizQuality, e);
    std::lock_guard<std::mutex> lk(mu_);
    if (!ok && err_.empty()) err_ = e.empty() ? "viz write failed" : e;
    free_.push_back(j.buf);
    cv_free_.notify_one();
  }
}

}  // namespace dpe_host
