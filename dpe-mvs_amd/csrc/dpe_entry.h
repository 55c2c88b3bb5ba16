// dpe_entry.h -- what every unit of the library needs to write an entry point of include/dpe_mvs.h:
// the thread's error string, the HIPC / TRY macros, roctx ranges and the prologue and waiting helpers
// of the concurrency contract.  Internal; the helpers are defined once, in dpe_mvs.hip, where the
// contract is stated.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>
#include <string>

#include "../../include/dpe_mvs.h"

namespace dpe {

extern thread_local std::string g_err;   // dpe_last_error: one per thread for the whole library

// roctx ranges (SURVEY.md §5 tracing): host-side enqueue regions of the pass, visible in
// `rocprofv3 --marker-trace` beside the kernel trace
struct Range {
  explicit Range(const char* m) { roctxRangePushA(m); }
  ~Range() { roctxRangePop(); }
  Range(const Range&) = delete;
  Range& operator=(const Range&) = delete;
};

// Host-waits for the work of the last dpe_pm_execute, which may have been enqueued on a caller
// stream: staging, fetching and freeing must not overwrite or release buffers that pass still uses.
hipError_t wait_pending(DpeContext* c);
// Host-waits until the context is quiet: the pending work, then everything on its own stream.
hipError_t host_wait(DpeContext* c);
// The stream an entry point enqueues on (the caller's, or the context's for nullptr), after making it
// wait for the pending work.
hipError_t enqueue_stream(DpeContext* c, void* caller_stream, hipStream_t* s);
// Makes the work enqueued on `s` so far the pending work that later calls wait for.
hipError_t mark_pending(DpeContext* c, hipStream_t s);
// The same for work that went on a caller's stream; the context's own stream orders its work itself.
hipError_t publish_foreign(DpeContext* c, hipStream_t s);
// The prologue of an entry point: clears the thread's error, refuses a null context or bad arguments
// with DPE_ERR_ARG and `bad_args`, and selects the context's device.
int enter(DpeContext* c, bool args_ok, const char* bad_args);

}  // namespace dpe

#define HIPC(expr)                                                                  \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                         \
      dpe::g_err = std::string(#expr) + ": " + hipGetErrorString(e_);               \
      return DPE_ERR_HIP;                                                           \
    }                                                                               \
  } while (0)

// a step of a longer sequence: its DPE_* code ends the caller unless it is DPE_OK
#define TRY(expr)                                                                   \
  do {                                                                              \
    if (const int rc_ = (expr); rc_ != DPE_OK) return rc_;                          \
  } while (0)
