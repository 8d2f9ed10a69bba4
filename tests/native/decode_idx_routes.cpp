// What a decode-idx device plan dispatches, on the CPU: rs_plan.cpp,
// rs_context.cpp and the kernel files compiled for the host only and linked against the
// recording HIP stand-ins (fake_hip_runtime.cpp, fake_hip_memory.cpp). Per case it prints the
// kernels one launch of the plan dispatched; tests/test_native_decode_idx.py checks that
//   - a decode-idx plan dispatches rs_merge_ragged once per group of 16 wanted rows, in the
//     smallest instance that holds the group's rows,
//   - merge mode and store mode dispatch different instances,
//   - a plan with nothing delivered dispatches nothing,
// and this program that only the delivered shards' and the wanted shards' pointers of stripes in
// the launch are in anything the plan uploaded, and what the plan reports of itself.
#include <algorithm>
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

// shard i of stripe b "lives" at an address nothing else holds
uint8_t* addr(int b, int i) {
  return reinterpret_cast<uint8_t*>(0x7a0000000000ull + (static_cast<uint64_t>(b) << 24) +
                                    (static_cast<uint64_t>(i) << 16));
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
  std::vector<int> expect, delivered, wanted;
};

bool has(const std::vector<int>& v, int i) { return std::find(v.begin(), v.end(), i) != v.end(); }

void run(rs_ctx* ctx, const char* name, int k, int m, const std::vector<Stripe>& st, bool store) {
  const int batch = static_cast<int>(st.size()), n = k + m;
  std::vector<size_t> sizes;
  std::vector<uint8_t> expect(static_cast<size_t>(batch) * n, 0);
  std::vector<const uint8_t*> input(expect.size(), nullptr);
  std::vector<uint8_t*> dst(expect.size(), nullptr);
  uint64_t bytes = 0;
  size_t rmax = 0;
  for (int b = 0; b < batch; ++b) {
    sizes.push_back(st[b].size);
    for (int i = 0; i < n; ++i) {
      const size_t at = static_cast<size_t>(b) * n + i;
      expect[at] = has(st[b].expect, i);
      if (has(st[b].delivered, i)) input[at] = addr(b, i);
      if (has(st[b].wanted, i)) dst[at] = addr(b, i);
    }
    if (!st[b].delivered.empty() && !st[b].wanted.empty()) {
      rmax = std::max(rmax, st[b].wanted.size());
      bytes += st[b].size * (st[b].delivered.size() + (store ? 1 : 2) * st[b].wanted.size());
    }
  }
  const int want_groups = static_cast<int>((rmax + 15) / 16);
  fake_mem::uploads().clear();
  rs_plan* plan = nullptr;
  CHECK(rs_plan_create_decode_idx(ctx, 0, k, m, batch, sizes.data(), expect.data(), input.data(), dst.data(),
                                  store ? RS_DECODE_IDX_STORE : 0u, &plan) == RS_OK);
  CHECK(plan);
  CHECK(rs_plan_groups(plan) == want_groups);
  int forms[4] = {-2, -2, -2, -2};
  CHECK(rs_plan_forms(plan, forms, 4) == want_groups);
  for (int g = 0; g < want_groups; ++g) CHECK(forms[g] == RS_ORDER_DECODE_IDX + RS_ORDER_CONSECUTIVE);
  CHECK(rs_plan_bytes(plan) == bytes);
  int orders[4] = {7, 7, 7, 7};
  CHECK(rs_plan_tune(plan, nullptr, 3, orders, 4) == RS_OK);
  for (int o : orders) CHECK(o == -1);
  const int none[2] = {-1, -1}, some[1] = {0};
  CHECK(rs_plan_set_orders(plan, none, want_groups) == RS_OK);
  if (want_groups) CHECK(rs_plan_set_orders(plan, some, 1) == RS_E_ARG);
  CHECK(rs_plan_launch_ceiling(plan, nullptr, RS_CEIL_READ) == RS_E_ARG);
  // of a stripe in the launch the delivered and the wanted pointers are uploaded; nothing else is
  for (int b = 0; b < batch; ++b) {
    const bool in_launch = !st[b].delivered.empty() && !st[b].wanted.empty();
    for (int i = 0; i < n; ++i)
      CHECK(uploaded(addr(b, i)) == (in_launch && (has(st[b].delivered, i) || has(st[b].wanted, i))));
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

std::vector<int> range(int a, int b) {
  std::vector<int> v;
  for (int i = a; i < b; ++i) v.push_back(i);
  return v;
}

}  // namespace

int main() {
  fake::device = 0;
  fake::bs_mode = 0;
  rs_ctx* ctx = nullptr;
  CHECK(rs_init(&ctx, 0) == RS_OK);
  const std::vector<int> mix = {0, 2, 3, 5, 6, 8, 9, 10, 12, 13};
  const std::vector<Stripe> st = {{8193, range(0, 10), {0}, {10, 11, 12, 13}},
                                  {40, range(4, 14), {}, {0, 1}},        // nothing delivered
                                  {20000, mix, {2, 3, 12, 13}, {1, 11}},
                                  {5, range(4, 14), {9}, {}}};           // nothing wanted
  run(ctx, "merge", 10, 4, st, false);
  run(ctx, "store", 10, 4, st, true);
  const std::vector<Stripe> st8 = {{8193, range(0, 10), {0, 9}, range(10, 18)}, {17, range(8, 18), {8}, {0}}};
  run(ctx, "merge-8", 10, 8, st8, false);
  run(ctx, "store-8", 10, 8, st8, true);
  // RS(10,20) with all 20 wanted: 16 rows, then 4; the second stripe has one row, in the first group alone
  const std::vector<Stripe> st20 = {{8193, range(0, 10), {3}, range(10, 30)}, {100, range(20, 30), {20, 29}, {5}}};
  run(ctx, "merge-two-groups", 10, 20, st20, false);
  run(ctx, "store-two-groups", 10, 20, st20, true);
  run(ctx, "nothing-delivered", 10, 4, {{8193, range(0, 10), {}, {10}}, {40, mix, {0}, {}}}, false);
  rs_shutdown(ctx);
  std::printf("decode_idx_routes ok\n");
  return 0;
}
