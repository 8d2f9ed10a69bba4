// What a decode-check device plan dispatches, on the CPU: rs_plan.cpp,
// rs_context.cpp and the kernel files compiled for the host only and linked against the
// recording HIP stand-ins (fake_hip_runtime.cpp, fake_hip_memory.cpp). Per case it prints the
// kernels one launch of the plan dispatched; tests/test_native_decode_check.py checks that
//   - a final plan dispatches rs_check_ragged once per group of 16 rows, in the smallest instance
//     that holds the group's rows, with different instances for merge and store,
//   - a non-final plan with check rows dispatches rs_merge_ragged,
//   - a plan made by rs_plan_create_decode_idx dispatches what it always did,
//   - a final stripe with nothing delivered is dispatched, a non-final one is not,
// and this program that the pointers of the stripes in the launch, and only they, are in what the
// plan uploaded (under FINAL|STORE a check pointer only marks the index, and is uploaded all the
// same: the kernel never loads it), and what the plan reports of itself.
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

// shard i of stripe b "lives" at an address nothing else holds; its accumulator at another
uint8_t* addr(int b, int i, bool acc = false) {
  return reinterpret_cast<uint8_t*>(0x7a0000000000ull + (static_cast<uint64_t>(b) << 24) +
                                    (static_cast<uint64_t>(i) << 16) + (acc ? 0x8000u : 0u));
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
  std::vector<int> expect, delivered, wanted, compared;
};

bool has(const std::vector<int>& v, int i) { return std::find(v.begin(), v.end(), i) != v.end(); }

void print_dispatches(const char* name, int groups) {
  std::printf("case %s: groups=%d\n", name, groups);
  size_t at = 0;
  while (at < fake::log.size()) {
    const size_t end = std::min(fake::log.find('\n', at), fake::log.size());
    const std::string line = fake::log.substr(at, end - at);
    at = end + 1;
    if (line.rfind("  attr ", 0) == 0 || line.rfind("  ", 0) != 0) continue;
    std::printf("dispatch %s\n", line.c_str() + 2);
  }
}

// flags: RS_DECODE_IDX_STORE | RS_DECODE_CHECK_FINAL; idx: through rs_plan_create_decode_idx (no
// compared shard then)
void run(rs_ctx* ctx, const char* name, int k, int m, const std::vector<Stripe>& st, unsigned flags,
         bool idx = false) {
  const int batch = static_cast<int>(st.size()), n = k + m;
  const bool store = flags & RS_DECODE_IDX_STORE, final = flags & RS_DECODE_CHECK_FINAL;
  std::vector<size_t> sizes;
  std::vector<uint8_t> expect(static_cast<size_t>(batch) * n, 0), in_launch(batch, 0);
  std::vector<const uint8_t*> input(expect.size(), nullptr);
  std::vector<uint8_t*> dst(expect.size(), nullptr), check(expect.size(), nullptr);
  uint64_t bytes = 0;
  size_t rmax = 0;
  for (int b = 0; b < batch; ++b) {
    sizes.push_back(st[b].size);
    for (int i = 0; i < n; ++i) {
      const size_t at = static_cast<size_t>(b) * n + i;
      expect[at] = has(st[b].expect, i);
      if (has(st[b].delivered, i)) input[at] = addr(b, i);
      if (has(st[b].wanted, i)) dst[at] = addr(b, i);
      if (has(st[b].compared, i)) check[at] = addr(b, i, true);
    }
    const size_t w = st[b].wanted.size(), x = st[b].compared.size();
    in_launch[b] = (!st[b].delivered.empty() && w + x > 0) || (final && x > 0);
    if (!in_launch[b]) continue;
    rmax = std::max(rmax, w + x);
    bytes += st[b].size * (st[b].delivered.size() + (store ? 1 : 2) * w +
                           (final ? (store ? 0 : 1) : (store ? 1 : 2)) * x);
  }
  const int want_groups = static_cast<int>((rmax + 15) / 16);
  fake_mem::uploads().clear();
  rs_plan* plan = nullptr;
  if (idx)
    CHECK(rs_plan_create_decode_idx(ctx, 0, k, m, batch, sizes.data(), expect.data(), input.data(), dst.data(), flags,
                                    &plan) == RS_OK);
  else
    CHECK(rs_plan_create_decode_check(ctx, 0, k, m, batch, sizes.data(), expect.data(), input.data(), dst.data(),
                                      check.data(), flags, &plan) == RS_OK);
  CHECK(plan);
  CHECK(rs_plan_groups(plan) == want_groups);
  int forms[4] = {-2, -2, -2, -2};
  CHECK(rs_plan_forms(plan, forms, 4) == want_groups);
  for (int g = 0; g < want_groups; ++g)
    CHECK(forms[g] == (final ? RS_ORDER_DECODE_CHECK : RS_ORDER_DECODE_IDX) + RS_ORDER_CONSECUTIVE);
  CHECK(rs_plan_bytes(plan) == bytes);
  int orders[4] = {7, 7, 7, 7};
  CHECK(rs_plan_tune(plan, nullptr, 3, orders, 4) == RS_OK);
  for (int o : orders) CHECK(o == -1);
  const int none[2] = {-1, -1}, some[1] = {0};
  CHECK(rs_plan_set_orders(plan, none, want_groups) == RS_OK);
  if (want_groups) CHECK(rs_plan_set_orders(plan, some, 1) == RS_E_ARG);
  CHECK(rs_plan_launch_ceiling(plan, nullptr, RS_CEIL_READ) == RS_E_ARG);
  CHECK(rs_plan_launch_ceiling(plan, nullptr, RS_CEIL_WRITE) == RS_E_ARG);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < n; ++i) {
      CHECK(uploaded(addr(b, i)) == (in_launch[b] && (has(st[b].delivered, i) || has(st[b].wanted, i))));
      CHECK(uploaded(addr(b, i, true)) == (in_launch[b] && !idx && has(st[b].compared, i)));
    }
  fake::log.clear();
  CHECK(rs_plan_launch(plan, nullptr) == RS_OK);
  print_dispatches(name, want_groups);
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
  const unsigned kStore = RS_DECODE_IDX_STORE, kFinal = RS_DECODE_CHECK_FINAL;
  const std::vector<int> mix = {0, 2, 3, 5, 6, 8, 9, 10, 12, 13};
  const std::vector<Stripe> st = {{8193, range(0, 10), {0, 12}, {10, 11}, {12, 13}},
                                  {40, range(4, 14), {}, {0, 1}, {}},      // nothing delivered, no check row
                                  {20000, mix, {2, 3, 12, 13}, {1}, {11}},
                                  {5, range(4, 14), {9}, {}, {}}};         // no row
  run(ctx, "final-merge", 10, 4, st, kFinal);
  run(ctx, "final-store", 10, 4, st, kFinal | kStore);
  run(ctx, "merge", 10, 4, st, 0);
  run(ctx, "store", 10, 4, st, kStore);
  const std::vector<Stripe> st8 = {{8193, range(0, 10), {0, 9, 17}, range(10, 14), range(14, 18)},
                                   {17, range(8, 18), {8}, {}, {0}}};
  run(ctx, "final-merge-8", 10, 8, st8, kFinal);
  run(ctx, "final-store-8", 10, 8, st8, kFinal | kStore);
  // RS(10,20): 12 wanted and 8 compared rows, 16 then 4; the second stripe has one row
  const std::vector<Stripe> st20 = {{8193, range(0, 10), {3, 29}, range(10, 22), range(22, 30)},
                                    {100, range(20, 30), {20, 29}, {}, {5}}};
  run(ctx, "final-merge-two-groups", 10, 20, st20, kFinal);
  run(ctx, "final-store-two-groups", 10, 20, st20, kFinal | kStore);
  run(ctx, "merge-two-groups", 10, 20, st20, 0);
  // nothing delivered anywhere: a final plan scans the stripe with a check row, a non-final plan
  // has nothing to do
  const std::vector<Stripe> idle = {{8193, range(0, 10), {}, {10}, {12}}, {40, mix, {}, {1}, {}}};
  run(ctx, "final-nothing-delivered", 10, 4, idle, kFinal);
  run(ctx, "nothing-delivered", 10, 4, idle, 0);
  // decode-idx plans, as before
  const std::vector<Stripe> sti = {{8193, range(0, 10), {0}, {10, 11, 12, 13}, {}}, {20000, mix, {2, 3}, {1, 11}, {}}};
  run(ctx, "idx-merge", 10, 4, sti, 0, true);
  run(ctx, "idx-store", 10, 4, sti, kStore, true);
  rs_shutdown(ctx);
  std::printf("decode_check_routes ok\n");
  return 0;
}
