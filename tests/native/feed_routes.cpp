// What a feed object dispatches, on the CPU: rs_plan.cpp, rs_context.cpp and the
// kernel files compiled for the host only and linked against the recording HIP stand-ins
// (fake_hip_runtime.cpp, fake_hip_memory.cpp). The allocation and synchronisation calls of the
// stand-ins are wrapped at link time (-Wl,--wrap) and counted here. Per case it prints one line
// per launch with the shard size and the kernel the launch dispatched;
// tests/test_native_feed.py checks that
//   - every launch dispatches rs_feed once, in the smallest instance that holds the rows,
//   - merge and store launches dispatch different instances,
//   - the grid is ceil(S / T) blocks of 256 threads with no LDS,
//   - a session feed dispatches rs_feed once, the first feed storing and the later ones merging,
// and this program that rs_feed_launch allocates, frees, copies and synchronises nothing, that
// create uploads once, that a launch of an index that is neither expected nor compared, an unknown
// flag bit and a NULL source are refused without a dispatch, and that a feed object without rows
// dispatches nothing; and of a session (rs_session.cpp linked in as well) that a feed enqueues no
// copy on the in-place route and one H2D on the staged route, that nothing comes back from the
// device before finish, and that finish runs one final launch and copies the wanted rows out.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/callfs_rs.h"
#include "fake_hip_memory.hpp"
#include "fake_hip_runtime.hpp"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {
long g_allocs = 0, g_frees = 0, g_syncs = 0;
}

extern "C" {
hipError_t __real_hipMalloc(void**, size_t);
hipError_t __real_hipHostMalloc(void**, size_t, unsigned);
hipError_t __real_hipFree(void*);
hipError_t __real_hipHostFree(void*);
hipError_t __real_hipStreamSynchronize(hipStream_t);
hipError_t __real_hipEventSynchronize(hipEvent_t);
hipError_t __wrap_hipMalloc(void** p, size_t n) {
  ++g_allocs;
  return __real_hipMalloc(p, n);
}
hipError_t __wrap_hipHostMalloc(void** p, size_t n, unsigned f) {
  ++g_allocs;
  return __real_hipHostMalloc(p, n, f);
}
hipError_t __wrap_hipFree(void* p) {
  ++g_frees;
  return __real_hipFree(p);
}
hipError_t __wrap_hipHostFree(void* p) {
  ++g_frees;
  return __real_hipHostFree(p);
}
hipError_t __wrap_hipStreamSynchronize(hipStream_t s) {
  ++g_syncs;
  return __real_hipStreamSynchronize(s);
}
hipError_t __wrap_hipEventSynchronize(hipEvent_t e) {
  ++g_syncs;
  return __real_hipEventSynchronize(e);
}
}

namespace {

// shard i "lives" at an address nothing else holds
uint8_t* addr(int i) { return reinterpret_cast<uint8_t*>(0x7a0000000000ull + (static_cast<uint64_t>(i) << 24)); }

struct Counters {
  long allocs, frees, syncs, h2d, d2h;
  size_t uploads;
  bool operator==(const Counters& o) const {
    return allocs == o.allocs && frees == o.frees && syncs == o.syncs && h2d == o.h2d && d2h == o.d2h &&
           uploads == o.uploads;
  }
};

Counters counters() {
  return {g_allocs, g_frees, g_syncs, fake_mem::async_copies().h2d, fake_mem::async_copies().d2h,
          fake_mem::uploads().size()};
}

// the dispatch lines of fake::log
std::vector<std::string> dispatches() {
  std::vector<std::string> out;
  size_t at = 0;
  while (at < fake::log.size()) {
    const size_t end = std::min(fake::log.find('\n', at), fake::log.size());
    const std::string line = fake::log.substr(at, end - at);
    at = end + 1;
    if (line.rfind("  attr ", 0) == 0 || line.rfind("  ", 0) != 0) continue;
    out.push_back(line.substr(2));
  }
  return out;
}

std::vector<int> range(int a, int b) {
  std::vector<int> v;
  for (int i = a; i < b; ++i) v.push_back(i);
  return v;
}

bool has(const std::vector<int>& v, int i) { return std::find(v.begin(), v.end(), i) != v.end(); }

void run(rs_ctx* ctx, const char* name, int k, int m, size_t S, const std::vector<int>& expect,
         const std::vector<int>& wanted, const std::vector<int>& compared) {
  const int n = k + m;
  std::vector<uint8_t> e(static_cast<size_t>(n), 0);
  std::vector<uint8_t*> dst(static_cast<size_t>(n), nullptr), chk(static_cast<size_t>(n), nullptr);
  for (int i = 0; i < n; ++i) {
    e[static_cast<size_t>(i)] = has(expect, i);
    if (has(wanted, i)) dst[static_cast<size_t>(i)] = addr(i);
    if (has(compared, i)) chk[static_cast<size_t>(i)] = addr(i);
  }
  const Counters c0 = counters();
  rs_feed* feed = nullptr;
  CHECK(rs_feed_create(ctx, 0, k, m, S, e.data(), dst.data(), chk.data(), &feed) == RS_OK);
  CHECK(feed);
  const Counters c1 = counters();
  CHECK(c1.uploads == c0.uploads + 1 && c1.allocs == c0.allocs + 1);  // one buffer, one upload
  std::printf("case %s: S=%zu rows=%zu\n", name, S, wanted.size() + compared.size());
  const uint8_t* src = addr(n + 1) + 3;
  // the first delivery stores, the others merge: an expected shard, then every compared one
  std::vector<int> order = {expect[expect.size() / 2]};
  order.insert(order.end(), compared.begin(), compared.end());
  order.push_back(expect.front());
  order.push_back(expect.back());
  for (size_t at = 0; at < order.size(); ++at) {
    fake::log.clear();
    CHECK(rs_feed_launch(feed, order[at], src, at == 0 ? RS_DECODE_IDX_STORE : 0u, nullptr) == RS_OK);
    const std::vector<std::string> d = dispatches();
    CHECK(d.size() == (wanted.empty() && compared.empty() ? 0u : 1u));
    for (const std::string& line : d) std::printf("dispatch %s %s\n", at == 0 ? "store" : "merge", line.c_str());
  }
  // refused, and nothing dispatched
  fake::log.clear();
  for (int i = 0; i < n; ++i)
    if (!has(expect, i) && !has(compared, i)) CHECK(rs_feed_launch(feed, i, src, 0, nullptr) == RS_E_ARG);
  CHECK(rs_feed_launch(feed, -1, src, 0, nullptr) == RS_E_ARG);
  CHECK(rs_feed_launch(feed, n, src, 0, nullptr) == RS_E_ARG);
  CHECK(rs_feed_launch(feed, expect[0], nullptr, 0, nullptr) == RS_E_ARG);
  CHECK(rs_feed_launch(feed, expect[0], src, 2u, nullptr) == RS_E_ARG);
  CHECK(rs_feed_launch(feed, expect[0], src, 0x80000001u, nullptr) == RS_E_ARG);
  CHECK(rs_feed_launch(nullptr, expect[0], src, 0, nullptr) == RS_E_ARG);
  CHECK(dispatches().empty());
  // no launch allocated, freed, copied or synchronised anything
  CHECK(counters() == c1);
  rs_feed_destroy(feed);
  CHECK(g_frees == c1.frees + 1);
}

// A session over RS(10,4) with one wanted and three compared shards, on the route
// CALLFS_RS_SESSION_INPLACE_MAX = `inplace_max` selects for S-byte shards.
void run_session(rs_ctx* ctx, const char* name, size_t S, const char* inplace_max, bool staged) {
  const int k = 10, m = 4, n = 14;
  setenv("CALLFS_RS_SESSION_INPLACE_MAX", inplace_max, 1);
  std::vector<uint8_t> e(n, 0), w(n, 0), c(n, 0);
  for (int i = 0; i < n; ++i) e[static_cast<size_t>(i)] = i == 0 || i >= 5;
  w[1] = 1;
  c[2] = c[3] = c[4] = 1;
  rs_session* s = nullptr;
  CHECK(rs_session_open(ctx, k, m, S, e.data(), w.data(), c.data(), RS_SESSION_CHECK, &s) == RS_OK && s);
  std::printf("case %s: S=%zu rows=4\n", name, S);
  std::vector<uint8_t> shard(S, 0x11);
  rs_host_counters h0{}, h1{};
  const int order[] = {7, 3, 0, 13, 2, 5, 6, 8, 9, 10, 11, 12, 4};
  int fed = 0;
  for (int idx : order) {
    const Counters c0 = counters();
    CHECK(rs_host_counters_read(ctx, &h0) == RS_OK);
    fake::log.clear();
    CHECK(rs_session_feed(s, idx, shard.data()) == RS_OK);
    const std::vector<std::string> d = dispatches();
    CHECK(d.size() == 1);
    std::printf("dispatch %s %s\n", fed == 0 ? "store" : "merge", d[0].c_str());
    const Counters c1 = counters();
    CHECK(c1.h2d == c0.h2d + (staged ? 1 : 0) && c1.d2h == c0.d2h && c1.uploads == c0.uploads);
    CHECK(rs_host_counters_read(ctx, &h1) == RS_OK);
    CHECK(h1.calls == h0.calls + 1 && h1.launches == h0.launches + 1 && h1.copies == h0.copies + (staged ? 1 : 0));
    // the ring's buffers are allocated by its first feeds alone
    if (fed >= 3) CHECK(c1.allocs == c0.allocs);
    CHECK(rs_session_feed(s, idx, shard.data()) == RS_E_ARG);  // a second feed of one index
    if (++fed == 5) {  // before the k-th expected shard
      std::vector<uint8_t*> none(n, nullptr);
      CHECK(rs_session_finish(s, none.data(), nullptr, nullptr, nullptr) == RS_E_TOO_FEW_SHARDS);
    }
  }
  CHECK(rs_session_feed(s, 1, shard.data()) == RS_E_ARG);  // wanted, not fed
  const Counters c0 = counters();
  std::vector<uint8_t> out(S, 0xee);
  std::vector<uint8_t*> dst(n, nullptr);
  dst[1] = out.data();
  uint64_t counts[15];
  fake::log.clear();
  CHECK(rs_session_finish(s, dst.data(), nullptr, nullptr, counts) == RS_OK);
  CHECK(dispatches().size() == 1 && dispatches()[0].find("rs_check_ragged") != std::string::npos);
  CHECK(counters().d2h == c0.d2h + 2);  // the status words and the wanted rows' span
  for (uint64_t v : counts) CHECK(v == 0);
  for (uint8_t b : out) CHECK(b == 0);  // the stand-in device ran nothing: the zeroed rows
  CHECK(rs_session_finish(s, dst.data(), nullptr, nullptr, counts) == RS_E_ARG);
  rs_session_close(s);
  unsetenv("CALLFS_RS_SESSION_INPLACE_MAX");
}

}  // namespace

int main() {
  fake::device = 0;
  fake::bs_mode = 0;
  rs_ctx* ctx = nullptr;
  CHECK(rs_init(&ctx, 0) == RS_OK);
  const std::vector<int> mix = {0, 2, 3, 5, 6, 8, 9, 10, 12, 13};
  run(ctx, "rows-4", 10, 4, 8211, range(0, 10), {10}, {11, 12, 13});
  run(ctx, "rows-4-wanted", 10, 4, 4096, range(4, 14), {0, 1, 2, 3}, {});
  run(ctx, "rows-2-mixed", 10, 4, 4097, mix, {1}, {11});
  run(ctx, "rows-1-tiny", 3, 2, 5, {0, 1, 2}, {}, {4});
  run(ctx, "rows-5", 10, 8, 40, range(0, 10), {10, 11}, {12, 13, 14});
  run(ctx, "rows-8", 10, 8, 12288, range(0, 10), range(10, 14), range(14, 18));
  run(ctx, "rows-9", 20, 12, 12289, range(0, 20), range(20, 25), range(25, 29));
  run(ctx, "rows-12", 20, 12, (1u << 20) + 1, range(12, 32), range(0, 6), range(6, 12));
  run(ctx, "rows-16", 10, 20, 65536, range(0, 10), range(10, 18), range(18, 26));
  run(ctx, "rows-0", 10, 4, 8211, range(0, 10), {}, {});
  run_session(ctx, "session-inplace", 8211, "8211", false);
  run_session(ctx, "session-staged", 8211, "8210", true);
  rs_shutdown(ctx);
  std::printf("feed_routes ok\n");
  return 0;
}
