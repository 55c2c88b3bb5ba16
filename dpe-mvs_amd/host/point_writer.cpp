// point_writer.cpp — see point_writer.h.
#include "point_writer.h"

namespace dpe_host {

PointCloudWriter::PointCloudWriter(DpeContext* ctx, int max_w, int max_h) : ctx_(ctx) {
  const size_t points = (size_t)max_w * max_h;
  bufs_.resize(kBuffers);
  for (int i = 0; i < kBuffers; ++i) {
    bufs_[i].resize(points);
    pinned_.push_back(dpe_host_pin(bufs_[i].data(), points * sizeof(FusedPoint)) == 0);   // refused: pageable, still works
    free_.push_back(i);
  }
  worker_ = std::thread([this]() { work(); });
}

bool PointCloudWriter::submit(int image_id, int mode, const DpeCamera& cam, const uint8_t* bgr, float dmin, float dmax,
                              const std::string& path, std::string& err) {
  int b;
  {
    std::unique_lock<std::mutex> lk(mu_);
    cv_free_.wait(lk, [this]() { return !free_.empty(); });
    b = free_.front(); free_.pop_front();
  }
  size_t n = 0;
  const int rc = dpe_state_point_cloud(ctx_, image_id, mode, &cam, bgr, dmin, dmax, bufs_[b].data(), bufs_[b].size(), &n, nullptr);
  std::lock_guard<std::mutex> lk(mu_);
  if (rc != 0) {
    err = std::string("point cloud failed: ") + dpe_last_error();
    free_.push_back(b);
    return false;
  }
  jobs_.push_back(Job{b, n, path});
  cv_job_.notify_one();
  return true;
}

bool PointCloudWriter::finish(std::string& err) {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_job_.notify_all();
  if (worker_.joinable()) worker_.join();
  for (size_t i = 0; i < bufs_.size(); ++i)
    if (pinned_[i]) { dpe_host_unpin(bufs_[i].data()); pinned_[i] = false; }
  err = err_;
  return err_.empty();
}

void PointCloudWriter::work() {
  for (;;) {
    Job j;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_job_.wait(lk, [this]() { return stop_ || !jobs_.empty(); });
      if (jobs_.empty()) return;
      j = std::move(jobs_.front()); jobs_.pop_front();
    }
    std::string e;
    bool ok = dpe_state_point_cloud_wait(ctx_, bufs_[j.buf].data()) == 0;
    if (!ok) e = std::string("point cloud failed: ") + dpe_last_error();
    else ok = export_point_cloud(j.path, bufs_[j.buf].data(), j.n, e);
    std::lock_guard<std::mutex> lk(mu_);
    if (!ok && err_.empty()) err_ = e.empty() ? "point cloud write failed" : e;
    free_.push_back(j.buf);
    cv_free_.notify_one();
  }
}

}  // namespace dpe_host
