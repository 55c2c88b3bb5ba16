// rank_group.h — the ranks of one pipeline run: the split of the problems, this rank's failure flag
// and the collectives that carry it.  No HIP, no files, no globals: the hooks of DpePipelineOptions
// are all it talks to.
//
// THE COLLECTIVE CONTRACT
//  * Every rank joins every collective, whatever happened to it locally.  A rank that returned early
//    would leave the others blocked in their all-gather, so with world > 1 a local error only raises
//    this rank's flag (fail()); the rank goes on to the next collective with empty work.
//  * The flag travels with the payload: exchange() appends one status float to every rank's message,
//    status_exchange() sends the flag alone.  Every rank therefore sees a failure at the same
//    collective, and all return 1 there together: the failing rank with its own first error, the
//    others with "rank R failed" (R the lowest failing rank).
//  * An error after a status step, between it and the payload collective the ranks are then committed
//    to, cannot stop the others any more.  The rank still joins that collective, records the error
//    with fail() and reports it at the next exchange's status step, or at the final status exchange
//    that every rank runs after its passes (so no rank returns 0 while another failed).
//  * A collective whose hook itself returns non-zero ends the run on this rank at once ("all-gather
//    failed").  Peers may be waiting in theirs: the optional abort hook (ncclCommAbort in bin/dpe)
//    makes them fail fast instead of waiting for their backend's timeout.  Without one (torch / gloo
//    hooks from Python) they wait for that timeout.
//  With world == 1 there is no collective and the caller returns at once on a failure.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "../../include/dpe_host.h"

namespace dpe_host {

class RankGroup {
 public:
  enum { kBeforeExchange = 0, kAfterExchange = 1 };   // fault_at's `when`

  // rank, world_size and the hooks of `opt`; reads DPE_FAULT_INJECT (so once per run, not per process)
  explicit RankGroup(const DpePipelineOptions& opt);

  int rank() const { return rank_; }
  int world() const { return world_; }
  bool multi() const { return world_ > 1; }
  bool has_device_hook() const { return gather_dev_ != nullptr; }

  // problems [r*n/world, (r+1)*n/world) to rank r (bench.py's images_per_rank is the same formula)
  void split(int n);
  const std::vector<int>& block(int r) const { return blocks_[r]; }
  const std::vector<int>& mine() const { return blocks_[rank_]; }
  size_t max_block() const { return max_block_; }   // maps per rank in an exchange: shorter blocks pad

  void fail(const std::string& msg) { if (!failed_) { failed_ = true; first_error_ = msg; } }
  bool failed() const { return failed_; }
  const std::string& first_error() const { return first_error_; }

  // The hooks themselves: false ("all-gather failed" in err, abort hook called) when one returns non-zero.
  bool gather(const float* send, size_t count, float* recv, std::string& err);
  bool gather_device(const float* dev_send, size_t count, float* dev_recv, std::string& err);
  // All-gather of send.size() floats per rank plus one status float, unpacked rank-major into recv;
  // false (err set) when any rank failed.
  bool exchange(std::vector<float>& send, std::vector<float>& recv, std::string& err);
  // The ranks' failure flags alone, one float each over the host hook; false (err set) when any rank failed.
  bool status_exchange(std::string& err);

  // DPE_FAULT_INJECT="before:R" / "after:R" (tests): true once, on rank R, at the first call with that
  // `when` (just before / after the first resident depth exchange's collectives).  Anything else never fires.
  bool fault_at(int when);
  static std::pair<int, int> parse_fault(const char* spec);   // (when, rank), (-1, -1) when malformed

 private:
  bool any_failed(const float* flags, size_t stride, std::string& err) const;
  bool hook_ok(int rc, std::string& err);   // a hook's return value: non-zero sets err and calls the abort hook

  int rank_, world_;
  dpe_allgather_fn gather_; void* gather_user_;
  dpe_allgather_dev_fn gather_dev_; void* gather_dev_user_;
  dpe_abort_fn abort_; void* abort_user_;
  std::vector<std::vector<int>> blocks_;
  size_t max_block_ = 0;
  bool failed_ = false;
  std::string first_error_;
  std::pair<int, int> fault_;
  bool fault_done_ = false;
};

}  // namespace dpe_host
