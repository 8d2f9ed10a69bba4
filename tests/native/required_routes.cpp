// The three routes of rs_plan_create_required on the CPU: rs_plan.cpp, rs_context.cpp and the
// kernel files compiled for the host only and linked against the recording HIP stand-ins
// (fake_hip_runtime.cpp, fake_hip_memory.cpp). Per case it prints the kernels a launch of the
// plan dispatched; tests/test_native_required_routes.py checks that
//   - required == NULL and an all-wanted set dispatch the ragged kernel,
//   - one size with one (mask, wanted) pair dispatches a uniform kernel (no per-stripe tables),
//   - anything else dispatches rs_apply_ragged_some, once per launch group that has a stripe,
//   - a plan without rows (uniform or required) dispatches nothing, and
//   - no pointer of an unwanted missing shard is anywhere in what the plan uploaded.
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

// shard i of stripe b "lives" at a recognisable address that nothing else holds
uint8_t* shard_addr(int b, int i) {
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
  std::vector<int> lost, wanted;
};

void run(rs_ctx* ctx, const char* name, int k, int m, const std::vector<Stripe>& st,
         bool null_required, int want_groups, int want_form) {
  const int n = k + m, batch = static_cast<int>(st.size());
  std::vector<size_t> sizes;
  std::vector<uint8_t> pres(static_cast<size_t>(batch) * n, 1), req(static_cast<size_t>(batch) * n, 0);
  std::vector<uint8_t*> shards;
  for (int b = 0; b < batch; ++b) {
    sizes.push_back(st[b].size);
    for (int i : st[b].lost) pres[static_cast<size_t>(b) * n + i] = 0;
    for (int i : st[b].wanted) req[static_cast<size_t>(b) * n + i] = 1;
    for (int i = 0; i < n; ++i) shards.push_back(shard_addr(b, i));
  }
  fake_mem::uploads().clear();
  rs_plan* plan = nullptr;
  CHECK(rs_plan_create_required(ctx, 0, k, m, batch, sizes.data(), pres.data(),
                                null_required ? nullptr : req.data(), shards.data(), &plan) == RS_OK);
  CHECK(plan);
  CHECK(rs_plan_groups(plan) == want_groups);
  int forms[4] = {-2, -2, -2, -2};
  CHECK(rs_plan_forms(plan, forms, 4) == want_groups);
  for (int g = 0; g < want_groups; ++g)
    if (want_form >= 0) CHECK(forms[g] == want_form);
  uint64_t bytes = 0;
  for (int b = 0; b < batch; ++b) {
    size_t w = 0;
    for (int i : st[b].lost)
      for (int j : st[b].wanted) w += i == j;
    if (null_required) w = st[b].lost.size();
    const size_t c = static_cast<size_t>(m) - st[b].lost.size();
    if (w + c) bytes += st[b].size * (k + w + c);
  }
  CHECK(rs_plan_bytes(plan) == bytes);
  // an unwanted missing shard's pointer is in nothing the plan uploaded; the others' are
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < n; ++i) {
      bool lost = false, wanted = null_required;
      for (int j : st[b].lost) lost |= i == j;
      for (int j : st[b].wanted) wanted |= i == j;
      if (lost && !wanted) CHECK(!uploaded(shard_addr(b, i)));
      if (lost && wanted) CHECK(uploaded(shard_addr(b, i)));
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
  fake::bs_mode = 0;  // the uniform route on the nibble-table and v_perm kernels
  rs_ctx* ctx = nullptr;
  CHECK(rs_init(&ctx, 0) == RS_OK);
  const int k = 10, m = 4;
  const std::vector<Stripe> mixed = {{8193, {0, 12}, {0}}, {40, {1}, {}}, {20000, {2, 3, 4, 5}, {2, 5}},
                                     {5, {0, 1, 2, 13}, {}}};
  std::vector<Stripe> all = mixed;
  for (Stripe& s : all) s.wanted = s.lost;
  run(ctx, "null", k, m, mixed, true, 1, RS_ORDER_RAGGED);
  run(ctx, "all-wanted", k, m, all, false, 1, RS_ORDER_RAGGED);
  run(ctx, "uniform", k, m, {{8193, {0, 12}, {0, 5}}, {8193, {0, 12}, {0, 7}}}, false, 1, -1);
  run(ctx, "uniform-no-rows", k, m, {{8193, {0, 1, 12, 13}, {5}}, {8193, {0, 1, 12, 13}, {}}}, false, 0, -1);
  run(ctx, "required", k, m, mixed, false, 1, RS_ORDER_REQUIRED);
  run(ctx, "required-no-rows", k, m, {{100, {0, 1, 12, 13}, {}}, {9000, {2, 3, 4, 5}, {}}}, false, 0, -1);
  // RS(3,20): 16 + 4 rows; the second launch group holds stripes 0 and 2 alone
  run(ctx, "required-two-groups", 3, 20,
      {{8193, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20},
        {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20}},
       {40000, {1, 2, 3, 4}, {}},
       {40000, {1}, {1}},
       {16, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20}, {}}},
      false, 2, RS_ORDER_REQUIRED);
  rs_shutdown(ctx);
  std::printf("required_routes ok\n");
  return 0;
}
