// Drives RankGroup (host/rank_group.cpp: the multi-rank split, failure flag and collectives of the
// host pipeline) with three ranks on three threads of one process over an in-process all-gather.
// Built under ASan + UBSan and under TSan (tests/test_sanitizers.py); links nothing else.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../dpe-mvs_amd/host/rank_group.h"

using dpe_host::RankGroup;

static std::atomic<int> g_bad{0};
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) { std::fprintf(stderr, "rank sanitize: line %d: %s\n", __LINE__, #cond); g_bad++; } \
  } while (0)

constexpr int kWorld = 3;

// all-gather of kWorld threads: the last to arrive opens the round, the last to leave closes it
struct Bus {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<float> buf;
  int inside = 0;
  bool draining = false;
};
struct Port {
  Bus* bus;
  int rank;
  bool hook_fails = false;
  int aborts = 0;
};

static int gather_hook(void* user, const float* send, size_t count, float* recv) {
  Port* p = static_cast<Port*>(user);
  if (p->hook_fails) return -1;
  Bus& b = *p->bus;
  std::unique_lock<std::mutex> lk(b.mu);
  b.cv.wait(lk, [&] { return !b.draining; });
  if (b.inside == 0) b.buf.assign(kWorld * count, -1.0f);
  std::memcpy(b.buf.data() + p->rank * count, send, count * sizeof(float));
  if (++b.inside == kWorld) { b.draining = true; b.cv.notify_all(); }
  else b.cv.wait(lk, [&] { return b.draining; });
  std::memcpy(recv, b.buf.data(), kWorld * count * sizeof(float));
  if (--b.inside == 0) { b.draining = false; b.cv.notify_all(); }
  return 0;
}
static int abort_hook(void* user) { static_cast<Port*>(user)->aborts++; return 0; }

static DpePipelineOptions options(int rank, int world, Port* port) {
  DpePipelineOptions o;
  std::memset(&o, 0, sizeof(o));
  o.rank = rank; o.world_size = world;
  o.allgather = gather_hook; o.allgather_user = port;
  o.abort_collectives = abort_hook; o.abort_user = port;
  return o;
}

// `body(group, port)` on kWorld threads, each with a fresh RankGroup (the failure flag is sticky)
template <class F>
static void on_three_ranks(bool hook_fails, F body) {
  Bus bus;
  Port ports[kWorld];
  std::vector<std::unique_ptr<RankGroup>> groups;
  for (int r = 0; r < kWorld; ++r) {
    ports[r] = Port{&bus, r, hook_fails, 0};
    groups.emplace_back(new RankGroup(options(r, kWorld, &ports[r])));
  }
  std::vector<std::thread> threads;
  for (int r = 0; r < kWorld; ++r) threads.emplace_back([&, r] { body(*groups[r], ports[r]); });
  for (auto& t : threads) t.join();
}

static void check_failure(const RankGroup& g, bool ok, const std::string& err) {
  CHECK(!ok);
  CHECK(err == (g.rank() == 1 ? "x" : "rank 1 failed"));
}

int main() {
  // the block split
  const int splits[3][2] = {{4, 3}, {16, 8}, {5, 5}};
  for (const auto& s : splits) {
    const int n = s[0], world = s[1];
    RankGroup g(options(world - 1, world, nullptr));
    g.split(n);
    size_t biggest = 0;
    for (int r = 0; r < world; ++r) {
      const std::vector<int>& b = g.block(r);
      CHECK((int)b.size() == (r + 1) * n / world - r * n / world);
      for (size_t k = 0; k < b.size(); ++k) CHECK(b[k] == r * n / world + (int)k);
      biggest = std::max(biggest, b.size());
    }
    CHECK(g.max_block() == biggest);
    CHECK(&g.mine() == &g.block(world - 1));
  }

  // a clean exchange: rank-major payloads, the status floats stripped, `send` as it was
  on_three_ranks(false, [](RankGroup& g, Port&) {
    std::vector<float> send{g.rank() * 10.0f, g.rank() * 10.0f + 1.0f}, recv;
    std::string err;
    CHECK(g.exchange(send, recv, err));
    CHECK(send.size() == 2 && recv.size() == 2 * kWorld && err.empty());
    for (int r = 0; r < kWorld && recv.size() == 2 * kWorld; ++r) CHECK(recv[2 * r] == r * 10.0f && recv[2 * r + 1] == r * 10.0f + 1.0f);
    CHECK(g.status_exchange(err) && err.empty());
    CHECK(!g.failed());
  });

  // rank 1 failed before an exchange: every rank stops there, rank 1 with its own (first) error
  on_three_ranks(false, [](RankGroup& g, Port& p) {
    if (g.rank() == 1) { g.fail("x"); g.fail("y"); }
    std::vector<float> send(5, 1.0f), recv;
    std::string err;
    const bool ok = g.exchange(send, recv, err);
    check_failure(g, ok, err);
    CHECK(recv.size() == 5 * kWorld && p.aborts == 0);
  });
  on_three_ranks(false, [](RankGroup& g, Port& p) {
    if (g.rank() == 1) g.fail("x");
    std::string err;
    const bool ok = g.status_exchange(err);
    check_failure(g, ok, err);
    CHECK(p.aborts == 0);
  });

  // the hook itself fails on every rank: the error, and one call of the abort hook
  on_three_ranks(true, [](RankGroup& g, Port& p) {
    std::vector<float> send(3, 0.0f), recv;
    std::string err;
    CHECK(!g.exchange(send, recv, err));
    CHECK(err == "all-gather failed" && p.aborts == 1);
  });

  // DPE_FAULT_INJECT: once, on the named rank, at the named point
  setenv("DPE_FAULT_INJECT", "before:1", 1);
  for (int r = 0; r < kWorld; ++r) {
    RankGroup g(options(r, kWorld, nullptr));
    CHECK(!g.fault_at(RankGroup::kAfterExchange));
    CHECK(g.fault_at(RankGroup::kBeforeExchange) == (r == 1));
    CHECK(!g.fault_at(RankGroup::kBeforeExchange));
  }
  CHECK(RankGroup::parse_fault("after:2") == std::make_pair((int)RankGroup::kAfterExchange, 2));
  for (const char* bad : {"", "before", "before:", ":1", "during:1", "before:x", "before:1x", "before:-1", "after:99999999999"}) {
    CHECK(RankGroup::parse_fault(bad).first < 0);
    setenv("DPE_FAULT_INJECT", bad, 1);
    for (int r = 0; r < kWorld; ++r) {
      RankGroup g(options(r, kWorld, nullptr));
      CHECK(!g.fault_at(RankGroup::kBeforeExchange) && !g.fault_at(RankGroup::kAfterExchange));
    }
  }
  unsetenv("DPE_FAULT_INJECT");
  CHECK(RankGroup::parse_fault(nullptr).first < 0);

  if (g_bad) return 1;
  std::printf("rank group sanitize ok\n");
  return 0;
}
