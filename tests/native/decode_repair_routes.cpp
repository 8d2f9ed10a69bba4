// What a decode-repair device plan dispatches, on the CPU: rs_plan.cpp,
// rs_context.cpp and the kernel files compiled for the host only and linked against the
// recording HIP stand-ins (fake_hip_runtime.cpp, fake_hip_memory.cpp). Per case it prints the
// kernels one launch of the plan dispatched; tests/test_native_decode_repair.py checks that
//   - a repair plan dispatches rs_repair_ragged exactly once, in the smallest instance that holds
//     the rows, with different instances for merge and store,
//   - a stripe with nothing delivered is dispatched,
//   - decode-check and decode-idx plans dispatch what they did before,
// and this program that the pointers of the stripes in the launch, and only they, fix pointers
// included, are in what the plan uploaded, what the plan reports of itself, and every refusal in
// the header's order through the C ABI.
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

// shard i of stripe b "lives" at an address nothing else holds; its accumulator and its fix
// buffer at others
uint8_t* addr(int b, int i, int kind = 0) {
  return reinterpret_cast<uint8_t*>(0x7a0000000000ull + (static_cast<uint64_t>(b) << 24) +
                                    (static_cast<uint64_t>(i) << 16) + static_cast<uint64_t>(kind) * 0x4000u);
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

// whether some upload holds exactly these pointers in consecutive slots
bool uploaded_run(const std::vector<const uint8_t*>& want) {
  const size_t bytes = want.size() * sizeof(void*);
  for (const auto& u : fake_mem::uploads())
    for (size_t at = 0; at + bytes <= u.size(); at += 8)
      if (std::memcmp(u.data() + at, want.data(), bytes) == 0) return true;
  return false;
}

struct Stripe {
  size_t size;
  std::vector<int> expect, delivered, wanted, compared, fix;
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

enum Kind { kRepair, kCheck, kIdx };

struct Arrays {
  std::vector<size_t> sizes;
  std::vector<uint8_t> expect;
  std::vector<const uint8_t*> input;
  std::vector<uint8_t*> dst, check, fix;
};

Arrays arrays(int k, int m, const std::vector<Stripe>& st) {
  const int batch = static_cast<int>(st.size()), n = k + m;
  Arrays a;
  a.expect.assign(static_cast<size_t>(batch) * n, 0);
  a.input.assign(a.expect.size(), nullptr);
  a.dst.assign(a.expect.size(), nullptr);
  a.check = a.fix = a.dst;
  for (int b = 0; b < batch; ++b) {
    a.sizes.push_back(st[b].size);
    for (int i = 0; i < n; ++i) {
      const size_t at = static_cast<size_t>(b) * n + i;
      a.expect[at] = has(st[b].expect, i);
      if (has(st[b].delivered, i)) a.input[at] = addr(b, i);
      if (has(st[b].wanted, i)) a.dst[at] = addr(b, i);
      if (has(st[b].compared, i)) a.check[at] = addr(b, i, 1);
      if (has(st[b].fix, i)) a.fix[at] = addr(b, i, 2);
    }
  }
  return a;
}

// flags: RS_DECODE_IDX_STORE (and RS_DECODE_CHECK_FINAL for a decode-check plan)
void run(rs_ctx* ctx, const char* name, int k, int m, const std::vector<Stripe>& st, unsigned flags, Kind kind) {
  const int batch = static_cast<int>(st.size()), n = k + m;
  const bool store = flags & RS_DECODE_IDX_STORE, final = kind == kRepair || (flags & RS_DECODE_CHECK_FINAL);
  Arrays a = arrays(k, m, st);
  std::vector<uint8_t> in_launch(batch, 0);
  uint64_t bytes = 0;
  size_t rmax = 0;
  for (int b = 0; b < batch; ++b) {
    const size_t w = st[b].wanted.size(), x = kind == kIdx ? 0 : st[b].compared.size();
    in_launch[b] = (!st[b].delivered.empty() && w + x > 0) || (final && x > 0);
    if (!in_launch[b]) continue;
    rmax = std::max(rmax, w + x);
    bytes += st[b].size * (st[b].delivered.size() + (store ? 1 : 2) * w +
                           (final ? (store ? 0 : 1) : (store ? 1 : 2)) * x);
  }
  const int want_groups = static_cast<int>((rmax + 15) / 16);
  fake_mem::uploads().clear();
  rs_plan* plan = nullptr;
  if (kind == kIdx)
    CHECK(rs_plan_create_decode_idx(ctx, 0, k, m, batch, a.sizes.data(), a.expect.data(), a.input.data(),
                                    a.dst.data(), flags, &plan) == RS_OK);
  else if (kind == kCheck)
    CHECK(rs_plan_create_decode_check(ctx, 0, k, m, batch, a.sizes.data(), a.expect.data(), a.input.data(),
                                      a.dst.data(), a.check.data(), flags, &plan) == RS_OK);
  else
    CHECK(rs_plan_create_decode_repair(ctx, 0, k, m, batch, a.sizes.data(), a.expect.data(), a.input.data(),
                                       a.dst.data(), a.check.data(), a.fix.data(), flags, &plan) == RS_OK);
  CHECK(plan);
  CHECK(rs_plan_groups(plan) == want_groups);
  if (kind == kRepair) CHECK(want_groups <= 1);
  int forms[4] = {-2, -2, -2, -2};
  CHECK(rs_plan_forms(plan, forms, 4) == want_groups);
  for (int g = 0; g < want_groups; ++g)
    CHECK(forms[g] == (kind == kRepair ? RS_ORDER_DECODE_REPAIR : final ? RS_ORDER_DECODE_CHECK : RS_ORDER_DECODE_IDX) +
                          RS_ORDER_CONSECUTIVE);
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
      CHECK(uploaded(addr(b, i, 1)) == (in_launch[b] && kind != kIdx && has(st[b].compared, i)));
      CHECK(uploaded(addr(b, i, 2)) == (in_launch[b] && kind == kRepair && has(st[b].fix, i)));
    }
  // the fix table, slot by slot: stripe b's k + 16 entries are the fix pointers of its expected
  // shards in ascending order, then of its compared shards in ascending order, then nulls
  for (int b = 0; kind == kRepair && b < batch; ++b) {
    if (!in_launch[b] || st[b].fix.empty()) continue;
    std::vector<int> e = st[b].expect, c = st[b].compared;
    std::sort(e.begin(), e.end());
    std::sort(c.begin(), c.end());
    std::vector<const uint8_t*> want(static_cast<size_t>(k) + 16, nullptr);
    for (size_t j = 0; j < e.size(); ++j)
      if (has(st[b].fix, e[j])) want[j] = addr(b, e[j], 2);
    for (size_t x = 0; x < c.size(); ++x)
      if (has(st[b].fix, c[x])) want[static_cast<size_t>(k) + x] = addr(b, c[x], 2);
    CHECK(uploaded_run(want));
  }
  std::vector<uint64_t> counts(static_cast<size_t>(batch) * (n + 1), 7);
  if (kind != kRepair) CHECK(rs_plan_blame(plan, nullptr, counts.data()) == RS_E_ARG);
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

// every refusal in the header's order, through the C ABI; nothing is created
void refusals(rs_ctx* ctx) {
  const int k = 10, m = 20;
  const Stripe good = {64, range(0, 10), {0, 19}, range(10, 18), range(18, 26), {0, 19}};
  auto create = [&](int kk, int mm, const std::vector<Stripe>& st, unsigned flags, int null = 0, rs_ctx* c = nullptr,
                    int batch = -1) {
    Arrays a = arrays(k, m, st);
    rs_plan* plan = reinterpret_cast<rs_plan*>(0x1);
    const int rc = rs_plan_create_decode_repair(
        c ? c : ctx, 0, kk, mm, batch < 0 ? static_cast<int>(st.size()) : batch, null == 1 ? nullptr : a.sizes.data(),
        null == 2 ? nullptr : a.expect.data(), null == 3 ? nullptr : a.input.data(), null == 4 ? nullptr : a.dst.data(),
        null == 5 ? nullptr : a.check.data(), null == 6 ? nullptr : a.fix.data(), flags, null == 7 ? nullptr : &plan);
    if (rc == RS_OK) rs_plan_destroy(plan);
    else CHECK(plan == nullptr || plan == reinterpret_cast<rs_plan*>(0x1));
    return rc;
  };
  Stripe few = good, many = good, in_wanted = good, chk_expected = good, fix_wanted = good, fix_unused = good,
         rows17 = good, zero = good;
  few.expect = range(0, 9);
  many.expect = range(0, 10);
  many.expect.push_back(29);
  in_wanted.delivered = {10};
  chk_expected.compared.push_back(3);
  fix_wanted.fix = {10};
  fix_unused.fix = {29};
  rows17.compared.push_back(26);
  zero.size = 0;
  Stripe rows17_zero = rows17, rows17_fix = rows17, few_all = few;
  rows17_zero.size = 0;
  rows17_fix.fix = {10};
  few_all.delivered = {10};
  few_all.fix = {10};
  few_all.compared.push_back(26);
  few_all.size = 0;
  CHECK(create(k, m, {good}, 0) == RS_OK && create(k, m, {good}, RS_DECODE_IDX_STORE) == RS_OK);
  // 1. the profile
  CHECK(create(0, m, {few_all}, 6, 1) == RS_E_INVALID_PROFILE && create(250, 10, {few_all}, 0) == RS_E_UNSUPPORTED);
  // 2. NULL arrays, the batch and the flag bits
  for (int null = 1; null <= 7; ++null) CHECK(create(k, m, {few_all}, 0, null) == RS_E_ARG);
  CHECK(create(k, m, {few_all}, 0, 0, nullptr, 0) == RS_E_ARG);
  for (unsigned bits : {2u, 3u, 4u, 0x80000000u}) CHECK(create(k, m, {few_all}, bits) == RS_E_ARG);
  // 3. the expect count
  CHECK(create(k, m, {few_all}, 0) == RS_E_TOO_FEW_SHARDS && create(k, m, {many}, 0) == RS_E_ARG);
  CHECK(create(k, m, {rows17_fix, few}, 0) == RS_E_TOO_FEW_SHARDS);
  // 4. a misplaced pointer, the fix placement included
  for (const Stripe& s : {in_wanted, chk_expected, fix_wanted, fix_unused, rows17_fix}) {
    CHECK(create(k, m, {s}, 0) == RS_E_ARG);
    CHECK(create(k, m, {rows17_zero, s}, 1) == RS_E_ARG);
  }
  // 5. the row limit, before a zero size
  CHECK(create(k, m, {rows17}, 0) == RS_E_UNSUPPORTED && create(k, m, {zero, rows17}, 0) == RS_E_UNSUPPORTED);
  CHECK(create(k, m, {rows17_zero}, 1) == RS_E_UNSUPPORTED);
  // 6. a zero size on a stripe in the launch
  CHECK(create(k, m, {good, zero}, 0) == RS_E_NO_DATA);
  // the siblings refuse the bits they refused
  Arrays a = arrays(k, m, {good});
  rs_plan* plan = nullptr;
  CHECK(rs_plan_create_decode_check(ctx, 0, k, m, 1, a.sizes.data(), a.expect.data(), a.input.data(), a.dst.data(),
                                    a.check.data(), 4, &plan) == RS_E_ARG);
  std::vector<const uint8_t*> noin(a.input.size(), nullptr);
  noin[0] = a.input[0];
  CHECK(rs_plan_create_decode_idx(ctx, 0, k, m, 1, a.sizes.data(), a.expect.data(), noin.data(), a.dst.data(), 2,
                                  &plan) == RS_E_ARG);
  CHECK(plan == nullptr);
}

}  // namespace

int main() {
  fake::device = 0;
  fake::bs_mode = 0;
  rs_ctx* ctx = nullptr;
  CHECK(rs_init(&ctx, 0) == RS_OK);
  refusals(ctx);
  const unsigned kStore = RS_DECODE_IDX_STORE, kFinal = RS_DECODE_CHECK_FINAL;
  const std::vector<int> mix = {0, 2, 3, 5, 6, 8, 9, 10, 12, 13};
  const std::vector<Stripe> st = {{8193, range(0, 10), {0, 12}, {10}, {11, 12, 13}, {0, 12, 3}},
                                  {40, range(4, 14), {}, {0, 1}, {}, {}},  // nothing delivered, no check row
                                  {20000, mix, {2, 3, 7}, {1}, {4, 7, 11}, {}},
                                  {5, range(4, 14), {9}, {}, {}, {9}}};     // no row
  run(ctx, "repair-merge", 10, 4, st, 0, kRepair);
  run(ctx, "repair-store", 10, 4, st, kStore, kRepair);
  const std::vector<Stripe> st8 = {{8193, range(0, 10), {0, 9, 17}, range(10, 14), range(14, 18), {17}},
                                   {17, range(8, 18), {8}, {}, {0}, {}}};
  run(ctx, "repair-merge-8", 10, 8, st8, 0, kRepair);
  run(ctx, "repair-store-8", 10, 8, st8, kStore, kRepair);
  // RS(10,20): 8 wanted and 8 compared rows beside a stripe with one row
  const std::vector<Stripe> st16 = {{8193, range(0, 10), {3, 29}, range(10, 18), range(22, 30), range(0, 10)},
                                    {100, range(20, 30), {20, 29}, {}, {5}, {5}}};
  run(ctx, "repair-merge-16", 10, 20, st16, 0, kRepair);
  run(ctx, "repair-store-16", 10, 20, st16, kStore, kRepair);
  // nothing delivered anywhere: the stripe with check rows is scanned
  const std::vector<Stripe> idle = {{8193, range(0, 10), {}, {10}, {11, 12, 13}, {11}}, {40, mix, {}, {1}, {}, {}}};
  run(ctx, "repair-nothing-delivered", 10, 4, idle, 0, kRepair);
  // decode-check and decode-idx plans, as before
  run(ctx, "final-merge", 10, 4, st, kFinal, kCheck);
  run(ctx, "final-store", 10, 4, st, kFinal | kStore, kCheck);
  run(ctx, "merge", 10, 4, st, 0, kCheck);
  const std::vector<Stripe> sti = {{8193, range(0, 10), {0}, {10, 11, 12, 13}, {}, {}}, {20000, mix, {2, 3}, {1, 11}, {}, {}}};
  run(ctx, "idx-merge", 10, 4, sti, 0, kIdx);
  run(ctx, "idx-store", 10, 4, sti, kStore, kIdx);
  rs_shutdown(ctx);
  std::printf("decode_repair_routes ok\n");
  return 0;
}
