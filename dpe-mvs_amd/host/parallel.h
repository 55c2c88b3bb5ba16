// parallel.h — the host thread count and the one spawn-and-join helper of libdpe_host.so.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <thread>
#include <vector>

namespace dpe_host {

// host threads of any pool: at most 16, the machine's, and OMP_NUM_THREADS when it is set (> 0)
inline int host_threads() {
  unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  if (const char* e = std::getenv("OMP_NUM_THREADS")) { const int v = std::atoi(e); if (v > 0) hw = std::min(hw, (unsigned)v); }
  return (int)std::min(16u, hw);
}

// fn(t) for t in [0, nt) on nt threads, joined before it returns (nt <= 1: on the calling thread).
// The caller partitions its items over t and caps nt by its item count.
template <class F>
void run_on_threads(int nt, F&& fn) {
  if (nt <= 1) { fn(0); return; }
  std::vector<std::thread> pool;
  pool.reserve(nt);
  for (int t = 0; t < nt; ++t) pool.emplace_back([&fn, t]() { fn(t); });
  for (auto& th : pool) th.join();
}

}  // namespace dpe_host
