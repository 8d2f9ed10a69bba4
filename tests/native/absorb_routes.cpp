// What an absorb object and an encode session dispatch, on the CPU: rs_plan.cpp,
// rs_context.cpp, rs_encode_session.cpp and the kernel files compiled for the host only and linked
// against the recording HIP stand-ins (fake_hip_runtime.cpp, fake_hip_memory.cpp). The allocation
// and synchronisation calls of the stand-ins are wrapped at link time (-Wl,--wrap) and counted
// here. Per case it prints one line per launch with the range and the kernel the launch
// dispatched; tests/test_native_absorb.py checks that
//   - every launch dispatches rs_absorb once, in the smallest instance that holds m,
//   - the grid is the sum of the intervals' ceil(columns / T) blocks of 256 threads with no LDS,
// and this program that rs_absorb_launch allocates, frees, copies and synchronises nothing, that
// create uploads once, that a NULL source, an empty range and a range outside [0, k * S) are
// refused without a dispatch; and of a session that a feed enqueues no copy on the in-place and
// the direct route and one H2D per piece on the staged route, that a feed of 2.5 slots makes three
// launches, that a refused feed launches nothing, that nothing comes back from the device before
// finish, and that finish launches nothing and copies the rows out.
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

// row j "lives" at an address nothing else holds
uint8_t* addr(int i) { return reinterpret_cast<uint8_t*>(0x7a0000000000ull + (static_cast<uint64_t>(i) << 28)); }

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

struct Range {
  uint64_t off, len;
};

void run(rs_ctx* ctx, const char* name, int k, int m, size_t S, const std::vector<Range>& ranges) {
  std::vector<uint8_t*> rows(static_cast<size_t>(m));
  for (int j = 0; j < m; ++j) rows[static_cast<size_t>(j)] = addr(j);
  const Counters c0 = counters();
  rs_absorb* ab = nullptr;
  CHECK(rs_absorb_create(ctx, 0, k, m, S, rows.data(), &ab) == RS_OK);
  CHECK(ab);
  const Counters c1 = counters();
  CHECK(c1.uploads == c0.uploads + 1 && c1.allocs == c0.allocs + 1);  // one buffer, one upload
  std::printf("case %s: k=%d m=%d S=%zu\n", name, k, m, S);
  const uint8_t* src = addr(m + 1) + 3;
  for (const Range& r : ranges) {
    fake::log.clear();
    CHECK(rs_absorb_launch(ab, r.off, r.len, src, nullptr) == RS_OK);
    const std::vector<std::string> d = dispatches();
    CHECK(d.size() == 1);
    std::printf("dispatch off=%llu len=%llu %s\n", static_cast<unsigned long long>(r.off),
                static_cast<unsigned long long>(r.len), d[0].c_str());
  }
  // refused, and nothing dispatched
  fake::log.clear();
  const uint64_t total = static_cast<uint64_t>(k) * S;
  CHECK(rs_absorb_launch(ab, 0, 0, src, nullptr) == RS_E_ARG);
  CHECK(rs_absorb_launch(ab, total, 1, src, nullptr) == RS_E_ARG);
  CHECK(rs_absorb_launch(ab, total - 1, 2, src, nullptr) == RS_E_ARG);
  CHECK(rs_absorb_launch(ab, 0, total + 1, src, nullptr) == RS_E_ARG);
  CHECK(rs_absorb_launch(ab, ~uint64_t{0}, 2, src, nullptr) == RS_E_ARG);
  CHECK(rs_absorb_launch(ab, 0, 1, nullptr, nullptr) == RS_E_ARG);
  CHECK(rs_absorb_launch(nullptr, 0, 1, src, nullptr) == RS_E_ARG);
  CHECK(dispatches().empty());
  // no launch allocated, freed, copied or synchronised anything
  CHECK(counters() == c1);
  rs_absorb_destroy(ab);
  CHECK(g_frees == c1.frees + 1);
}

enum class Route { kInPlace, kDirect, kStaged };

// A session over RS(10,4) and a body of L bytes, slots of `chunk` bytes, on the route
// CALLFS_RS_SESSION_INPLACE_MAX = `inplace_max` and the body's memory select.
void run_session(rs_ctx* ctx, const char* name, size_t L, const char* chunk, const char* inplace_max, Route route) {
  const int k = 10, m = 4;
  setenv("CALLFS_RS_SESSION_INPLACE_MAX", inplace_max, 1);
  setenv("CALLFS_RS_ENCODE_SESSION_CHUNK", chunk, 1);
  const size_t slot = std::min<size_t>(L, std::strtoull(chunk, nullptr, 0));
  const size_t S = (L + k - 1) / k;
  rs_encode_session* s = nullptr;
  CHECK(rs_encode_session_open(ctx, k, m, L, &s) == RS_OK && s);
  std::printf("case %s: k=%d m=%d S=%zu\n", name, k, m, S);
  // the body: at an odd offset inside an rs_host_alloc buffer for the direct route
  void* pinned = nullptr;
  std::vector<uint8_t> plain;
  uint8_t* body;
  if (route == Route::kDirect) {
    CHECK(rs_host_alloc(ctx, L + 64, &pinned) == RS_OK);
    body = static_cast<uint8_t*>(pinned) + 5;
  } else {
    plain.assign(L, 0);
    body = plain.data();
  }
  for (size_t x = 0; x < L; ++x) body[x] = static_cast<uint8_t>(x * 7 + 1);
  // 2.5 slots, then the head, then the rest in two feeds: every byte once
  const size_t a = slot / 2 + 3;
  const std::vector<Range> feeds = {{a, 2 * slot + slot / 2}, {0, a}, {a + 2 * slot + slot / 2, 11},
                                    {a + 2 * slot + slot / 2 + 11, L - (a + 2 * slot + slot / 2 + 11)}};
  std::vector<uint8_t*> parity(m);
  std::vector<std::vector<uint8_t>> pbuf(m, std::vector<uint8_t>(S, 0xee));
  for (int j = 0; j < m; ++j) parity[static_cast<size_t>(j)] = pbuf[static_cast<size_t>(j)].data();
  size_t shard = 0;
  rs_host_counters h0{}, h1{};
  const Counters start = counters();
  for (size_t at = 0; at < feeds.size(); ++at) {
    const Range& r = feeds[at];
    CHECK(r.len > 0 && r.off + r.len <= L);
    const long pieces = static_cast<long>((r.len + slot - 1) / slot);
    if (at == 0) CHECK(pieces == 3);
    const Counters c0 = counters();
    CHECK(rs_host_counters_read(ctx, &h0) == RS_OK);
    fake::log.clear();
    CHECK(rs_encode_session_feed(s, r.off, body + r.off, r.len) == RS_OK);
    const std::vector<std::string> d = dispatches();
    CHECK(static_cast<long>(d.size()) == pieces);
    uint64_t off = r.off;
    for (const std::string& line : d) {
      const uint64_t n = std::min<uint64_t>(slot, r.off + r.len - off);
      std::printf("dispatch off=%llu len=%llu %s\n", static_cast<unsigned long long>(off),
                  static_cast<unsigned long long>(n), line.c_str());
      off += n;
    }
    const Counters c1 = counters();
    const long staged = route == Route::kStaged ? pieces : 0;
    CHECK(c1.h2d == c0.h2d + staged && c1.d2h == c0.d2h && c1.uploads == c0.uploads);
    CHECK(rs_host_counters_read(ctx, &h1) == RS_OK);
    CHECK(h1.calls == h0.calls + 1 && h1.launches == h0.launches + static_cast<uint64_t>(pieces) &&
          h1.copies == h0.copies + static_cast<uint64_t>(staged));
    // the ring's buffers are allocated by its first pieces alone; the direct route has none
    if (route == Route::kDirect || at >= 1) CHECK(c1.allocs == c0.allocs);
    // refused, nothing launched: the same range again, an overlap, past the end, empty
    fake::log.clear();
    CHECK(rs_encode_session_feed(s, r.off, body + r.off, r.len) == RS_E_ARG);
    CHECK(rs_encode_session_feed(s, r.off + r.len - 1, body, 1) == RS_E_ARG);
    CHECK(rs_encode_session_feed(s, L - 1, body, 2) == RS_E_ARG);
    CHECK(rs_encode_session_feed(s, L, body, 1) == RS_E_ARG);
    CHECK(rs_encode_session_feed(s, 0, body, 0) == RS_E_ARG);
    CHECK(rs_encode_session_feed(s, 0, nullptr, 1) == RS_E_ARG);
    CHECK(dispatches().empty());
    if (at + 1 < feeds.size()) {  // before coverage: the session stays usable
      CHECK(rs_encode_session_finish(s, parity.data(), &shard) == RS_E_SHORT_DATA);
      CHECK(dispatches().empty());
    }
  }
  CHECK(counters().d2h == start.d2h);  // nothing came back before finish
  fake::log.clear();
  const Counters c0 = counters();
  CHECK(rs_encode_session_finish(s, parity.data(), &shard) == RS_OK && shard == S);
  CHECK(dispatches().empty());
  CHECK(counters().d2h == c0.d2h + 1);  // the rows' span through staging
  for (const auto& p : pbuf)
    for (uint8_t b : p) CHECK(b == 0);  // the stand-in device ran nothing: the zeroed rows
  CHECK(rs_encode_session_finish(s, parity.data(), nullptr) == RS_OK);  // a finish may be repeated
  CHECK(rs_encode_session_feed(s, 0, body, 1) == RS_E_ARG);               // feeds after it may not
  uint8_t peek[4];
  CHECK(rs_encode_session_peek(s, 0, peek, 4) == RS_OK && rs_encode_session_peek(s, m, peek, 1) == RS_E_ARG);
  CHECK(rs_encode_session_peek(s, -1, peek, 1) == RS_E_ARG && rs_encode_session_peek(s, 0, peek, S + 1) == RS_E_ARG);
  rs_encode_session_close(s);
  if (pinned) CHECK(rs_host_free(ctx, pinned) == RS_OK);
  unsetenv("CALLFS_RS_SESSION_INPLACE_MAX");
  unsetenv("CALLFS_RS_ENCODE_SESSION_CHUNK");
}

void open_refusals(rs_ctx* ctx) {
  rs_encode_session* s = nullptr;
  CHECK(rs_encode_session_open(ctx, 0, 4, 0, &s) == RS_E_INVALID_PROFILE);
  CHECK(rs_encode_session_open(nullptr, 200, 100, 0, nullptr) == RS_E_UNSUPPORTED);
  CHECK(rs_encode_session_open(nullptr, 10, 20, 0, &s) == RS_E_ARG);
  CHECK(rs_encode_session_open(ctx, 10, 20, 0, nullptr) == RS_E_ARG);
  CHECK(rs_encode_session_open(ctx, 10, 20, 0, &s) == RS_E_SHORT_DATA);
  CHECK(rs_encode_session_open(ctx, 10, 20, 1, &s) == RS_E_UNSUPPORTED);
  CHECK(rs_encode_session_open(ctx, 10, 17, 1, &s) == RS_E_UNSUPPORTED);
  CHECK(!s);
  rs_encode_session_close(nullptr);
}

}  // namespace

int main() {
  fake::device = 0;
  fake::bs_mode = 0;
  rs_ctx* ctx = nullptr;
  CHECK(rs_init(&ctx, 0) == RS_OK);
  const size_t T = 4096;
  // one shard; every shard at every column; three intervals; two shards with an empty middle
  // interval; a tail-only interval; one byte
  run(ctx, "rows-4", 10, 4, 8211, {{0, 8211}, {0, 82110}, {8209, 2 * 8211 + 5}, {8208, 8210}, {16, 15}, {82109, 1},
                                    {100, 9 * 8211}});
  run(ctx, "rows-4-tiny", 4, 2, 1, {{0, 2}, {1, 1}, {0, 4}});
  run(ctx, "rows-2", 3, 2, 5, {{0, 15}, {3, 7}, {4, 2}});
  run(ctx, "rows-3", 1, 3, T + 16, {{0, T + 16}, {1, T}, {T, 16}});
  run(ctx, "rows-8", 10, 8, T + 16, {{0, 10 * (T + 16)}, {T + 14, 2 * (T + 16) + 5}, {T + 13, T + 15}});
  run(ctx, "rows-12", 20, 12, 17, {{0, 340}, {15, 39}, {14, 16}});
  run(ctx, "rows-16", 64, 16, 2 * T + 83, {{0, 64 * (2 * T + 83)}, {2 * T + 81, 2 * (2 * T + 83) + 5}, {5, 262144}});
  open_refusals(ctx);
  run_session(ctx, "session-inplace", 10 * 8211 - 7, "8000", "8000", Route::kInPlace);
  run_session(ctx, "session-direct", 10 * 8211 - 7, "8000", "8000", Route::kDirect);
  run_session(ctx, "session-staged", 10 * 8211 - 7, "8000", "0", Route::kStaged);
  rs_shutdown(ctx);
  std::printf("absorb_routes ok\n");
  return 0;
}
