// What an update device plan dispatches, on the CPU: rs_plan.cpp,
// rs_context.cpp and the kernel files compiled for the host only and linked against the
// recording HIP stand-ins (fake_hip_runtime.cpp, fake_hip_memory.cpp). Per case it prints the
// kernels one launch of the plan dispatched; tests/test_native_update.py checks that
//   - an update plan dispatches rs_update_ragged once per group of 16 parity rows,
//   - pair mode and EncodeIdx mode dispatch different instances,
//   - an all-unchanged plan dispatches nothing,
// and this program that the pointers of unchanged shards are in nothing the plan uploaded.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

// (kind 0 old, 1 new, 2 parity) shard i of stripe b "lives" at an address nothing else holds
uint8_t* addr(int kind, int b, int i) {
  return reinterpret_cast<uint8_t*>(0x7a0000000000ull + (static_cast<uint64_t>(kind) << 36) +
                                    (static_cast<uint64_t>(b) << 24) + (static_cast<uint64_t>(i) << 16));
}

bool uploaded(const uint8_t* p) {
  for (const auto& u : fake_mem::uploads())
    for (size_t at = 0; at + sizeof p <= u.size(); at += 8) {
      const uint8_t* q;
      std::memcpy(&q, u.data() + at, sizeof q);
      if (q == p) return true;
    }
  return false;
}

struct Stripe {
  size_t size;
  std::vector<int> changed;
};

void run(rs_ctx* ctx, const char* name, int k, int m, const std::vector<Stripe>& st, bool pair) {
  const int batch = static_cast<int>(st.size());
  std::vector<size_t> sizes;
  std::vector<uint8_t> flags(static_cast<size_t>(batch) * k, 0);
  std::vector<const uint8_t*> old_data, new_data;
  std::vector<uint8_t*> parity;
  uint64_t bytes = 0;
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    sizes.push_back(st[b].size);
    for (int i : st[b].changed) flags[static_cast<size_t>(b) * k + i] = 1;
    for (int i = 0; i < k; ++i) {
      old_data.push_back(addr(0, b, i));
      new_data.push_back(addr(1, b, i));
    }
    for (int j = 0; j < m; ++j) parity.push_back(addr(2, b, j));
    if (!st[b].changed.empty()) {
      any = true;
      bytes += st[b].size * (st[b].changed.size() * (pair ? 2 : 1) + 2 * static_cast<size_t>(m));
    }
  }
  const int want_groups = any ? (m + 15) / 16 : 0;
  fake_mem::uploads().clear();
  rs_plan* plan = nullptr;
  CHECK(rs_plan_create_update(ctx, 0, k, m, batch, sizes.data(), flags.data(),
                              pair ? old_data.data() : nullptr, new_data.data(), parity.data(),
                              &plan) == RS_OK);
  CHECK(plan);
  CHECK(rs_plan_groups(plan) == want_groups);
  int forms[4] = {-2, -2, -2, -2};
  CHECK(rs_plan_forms(plan, forms, 4) == want_groups);
  for (int g = 0; g < want_groups; ++g) CHECK(forms[g] == RS_ORDER_UPDATE);
  CHECK(rs_plan_bytes(plan) == bytes);
  int orders[4] = {7, 7, 7, 7};
  CHECK(rs_plan_tune(plan, nullptr, 3, orders, 4) == RS_OK);
  for (int o : orders) CHECK(o == -1);
  CHECK(rs_plan_launch_ceiling(plan, nullptr, RS_CEIL_READ) == RS_E_ARG);
  // a changed shard's old (pair mode) and new pointers and its stripe's parity pointers are
  // uploaded; nothing of an unchanged shard or an unchanged stripe is
  for (int b = 0; b < batch; ++b) {
    for (int i = 0; i < k; ++i) {
      const bool ch = flags[static_cast<size_t>(b) * k + i] != 0;
      CHECK(uploaded(addr(1, b, i)) == ch);
      CHECK(uploaded(addr(0, b, i)) == (ch && pair));
    }
    for (int j = 0; j < m; ++j) CHECK(uploaded(addr(2, b, j)) == !st[b].changed.empty());
  }
  fake::log.clear();
  CHECK(rs_plan_launch(plan, nullptr) == RS_OK);
  std::printf("case %s: groups=%d\n", name, want_groups);
  size_t at = 0;
  while (at < fake::log.size()) {
    const size_t end = std::min(fake::log.find('\n', at), fake::log.size());
    const std::string line = fake::log.substr(at, end - at);
    at = end + 1;
    if (line.rfind("  attr ", 0) == 0 || line.rfind("  ", 0) != 0) continue;
    std::printf("dispatch %s\n", line.c_str() + 2);
  }
  rs_plan_destroy(plan);
}

}  // namespace

int main() {
  fake::device = 0;
  fake::bs_mode = 0;
  rs_ctx* ctx = nullptr;
  CHECK(rs_init(&ctx, 0) == RS_OK);
  const std::vector<Stripe> st = {{8193, {0}}, {40, {}}, {20000, {2, 3, 4, 5}}, {5, {9}}};
  run(ctx, "pair", 10, 4, st, true);
  run(ctx, "single", 10, 4, st, false);
  run(ctx, "pair-8", 10, 8, st, true);
  run(ctx, "pair-two-groups", 10, 20, st, true);
  run(ctx, "single-two-groups", 10, 20, st, false);
  run(ctx, "unchanged", 10, 4, {{8193, {}}, {40, {}}}, true);
  rs_shutdown(ctx);
  std::printf("update_routes ok\n");
  return 0;
}
