// rank_group.cpp — see rank_group.h for the contract these collectives keep.
#include "rank_group.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace dpe_host {

RankGroup::RankGroup(const DpePipelineOptions& opt)
    : rank_(opt.rank), world_(std::max(1, opt.world_size)),
      gather_(opt.allgather), gather_user_(opt.allgather_user),
      gather_dev_(opt.allgather_device), gather_dev_user_(opt.allgather_device_user),
      abort_(opt.abort_collectives), abort_user_(opt.abort_user),
      fault_(parse_fault(std::getenv("DPE_FAULT_INJECT"))) {}

void RankGroup::split(int n) {
  blocks_.assign(world_, {});
  max_block_ = 0;
  for (int r = 0; r < world_; ++r) {
    for (int i = r * n / world_; i < (r + 1) * n / world_; ++i) blocks_[r].push_back(i);
    max_block_ = std::max(max_block_, blocks_[r].size());
  }
}

bool RankGroup::hook_ok(int rc, std::string& err) {
  if (rc == 0) return true;
  err = "all-gather failed";
  if (abort_) (void)abort_(abort_user_);
  return false;
}

bool RankGroup::gather(const float* send, size_t count, float* recv, std::string& err) {
  return hook_ok(gather_(gather_user_, send, count, recv), err);
}

bool RankGroup::gather_device(const float* dev_send, size_t count, float* dev_recv, std::string& err) {
  return hook_ok(gather_dev_(gather_dev_user_, dev_send, count, dev_recv), err);
}

// the first set flag of flags[r * stride], r < world: err = this rank's own error or "rank R failed"
bool RankGroup::any_failed(const float* flags, size_t stride, std::string& err) const {
  for (int r = 0; r < world_; ++r)
    if (flags[(size_t)r * stride] != 0.0f) {
      err = r == rank_ ? first_error_ : "rank " + std::to_string(r) + " failed";
      return true;
    }
  return false;
}

bool RankGroup::exchange(std::vector<float>& send, std::vector<float>& recv, std::string& err) {
  const size_t per = send.size();
  send.push_back(failed_ ? 1.0f : 0.0f);
  recv.assign((per + 1) * world_, 0.0f);
  if (!gather(send.data(), per + 1, recv.data(), err)) return false;
  send.pop_back();
  std::vector<float> packed(per * world_);
  for (int r = 0; r < world_; ++r)
    std::memcpy(packed.data() + (size_t)r * per, recv.data() + (size_t)r * (per + 1), per * sizeof(float));
  const bool bad = any_failed(recv.data() + per, per + 1, err);
  recv.swap(packed);
  return !bad;
}

bool RankGroup::status_exchange(std::string& err) {
  const float flag = failed_ ? 1.0f : 0.0f;
  std::vector<float> all(world_, 0.0f);
  if (!gather(&flag, 1, all.data(), err)) return false;
  return !any_failed(all.data(), 1, err);
}

std::pair<int, int> RankGroup::parse_fault(const char* spec) {
  const std::pair<int, int> none(-1, -1);
  if (!spec) return none;
  const std::string v(spec);
  const size_t c = v.find(':');
  if (c == std::string::npos || c + 1 == v.size()) return none;
  const int when = v.compare(0, c, "before") == 0 ? kBeforeExchange : (v.compare(0, c, "after") == 0 ? kAfterExchange : -1);
  char* end = nullptr;
  const long r = std::strtol(v.c_str() + c + 1, &end, 10);
  if (when < 0 || *end != '\0' || r < 0 || r > 1 << 20) return none;
  return std::make_pair(when, (int)r);
}

bool RankGroup::fault_at(int when) {
  if (fault_done_ || fault_.first != when || fault_.second != rank_) return false;
  fault_done_ = true;
  return true;
}

}  // namespace dpe_host
