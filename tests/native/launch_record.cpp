// Records what rs_kernels.hip's dispatch does, on the CPU: linked against fake_hip_runtime.cpp
// and a host-only build of rs_kernels.hip, it runs a seeded sweep of launch shapes through
// launch_form, order_candidates, launch_apply and launch_ceiling and prints, per case, the
// case, the rule's form and a 64-bit hash of everything that was dispatched (kernel symbol,
// grid, block, LDS bytes, nvec, t_base, tail placement, byte-kernel tail0, event marking,
// the wide-LDS opt-in, the bit-sliced path). tests/test_native_launch_record.py compares that
// with tests/golden/launch_record/, which was recorded from the dispatch code as it stood
// before it was restructured: the restructured code must choose exactly the same launches.
//
//   launch_record [--stride N]   one line per case (every N-th case)
//   launch_record --full I       the whole record of case I
//   launch_record --unreached    registered kernels the sweep never dispatched
//   launch_record --time         ns per launch_apply (selection cost; recording off)
//   launch_record --wide         the kernel each wide-ring launch (R 9..16, consecutive and Q8,
//                                pinned and by the rule) dispatches with the bit-sliced path off
//
// The environment toggles of rs_kernels.hip are read once per process, so the test runs one
// process per setting.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bitslice.hpp"
#include "fake_hip_runtime.hpp"
#include "rs_kernels.hpp"
#include "tune_table.hpp"

using namespace callfs;

namespace {

constexpr int kCases = 600;
constexpr uint64_t kTile = 8192;

struct Case {
  ApplyArgs a{};
  bool bytes_only = false;
  int bs = 0;    // 0 no handle, 1 not compiled, 2 ready
  int mode = 1;  // bs::Mode
  bool events = false;
};

struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  template <class T, size_t N>
  T pick(const T (&v)[N]) { return v[next() % N]; }
  bool one_in(unsigned n) { return next() % n == 0; }
};

const int kKs[] = {1, 2, 3, 4, 5, 6, 7, 12, 13, 64, 65, 96, 97, 128, 129, 256};
const uint64_t kSs[] = {
    15, 16, 17, 31, 100, kTile, kTile + 7, 32 * kTile, 33 * kTile, 64 * kTile, 128 * kTile,
    129 * kTile, 256 * kTile, 257 * kTile, 512 * kTile, 513 * kTile, 1024 * kTile, 1025 * kTile,
    104858, 174763, 1048577, 5592406, 6710887,
    // S % 16 != 0 with the last tile's vectors on both sides of tail_code's last + 64 <= BS
    // (448 / 449 vectors in the last tile), at 4 tiles and beyond 32 tiles per stripe
    16 * (3 * 512 + 448) + 5, 16 * (3 * 512 + 449) + 5, 16 * (39 * 512 + 100) + 3,
    16 * (39 * 512 + 500) + 3, 16 * (31 * 512 + 448) + 9, 16 * (32 * 512 + 448) + 9};
const int kBatches[] = {1, 2, 7, 256, 1024, 70000};
const int kTzs[] = {0, 4, 12, 20, 24, 63};
const uint64_t kStrides[] = {0, 16ull << 20, 1ull << 20, 2ull << 20, 15ull * 1000 * 1000 + 4096};
const uint32_t kMis[][2] = {{0, 0}, {1, 0}, {2, 0}, {0, 1}, {1, 1}, {2, 2}};

uint32_t verify_mask(Rng& r, int R, int kind) {
  const uint32_t rows = (1u << R) - 1;
  switch (kind) {
    case 1: return 1u << (r.next() % R);
    case 2: return r.one_in(2) ? rows : ~0u;  // bits above R set as well
    case 3: return R == 1 ? 0x10000u : (rows >> 1) | (r.one_in(2) ? 0x30000u : 0u);
    default: return 0;
  }
}

ApplyArgs shape(int K, int R, uint64_t S, int batch) {
  ApplyArgs a{};
  a.in_tab = reinterpret_cast<const uint8_t* const*>(0x1000);
  a.out_tab = reinterpret_cast<uint8_t* const*>(0x2000);
  a.tabs = reinterpret_cast<const uint32_t*>(0x3000);
  a.ltabs = reinterpret_cast<const uint8_t*>(0x4000);
  a.status = reinterpret_cast<int*>(0x5000);
  a.status_stride = 1;
  a.S = S;
  a.K = K;
  a.R = R;
  a.batch = batch;
  return a;
}

Case make_case(int i) {
  Case c;
  Rng r{0x5eed0000ull + static_cast<uint64_t>(i)};
  if (i == 0) {  // a grid of more than twice the slice limit
    c.a = shape(10, 4, 1 << 20, 1024);
    c.a.addr_tz = 20;
    c.a.stripe_stride = 14ull << 20;
    return c;
  }
  if (i <= 4) {  // the v_perm kernel above 1024 tiles per stripe (its Q16 instances), R = i
    c.a = shape(3, i, 1025 * kTile, 2);
    c.a.addr_tz = 24;
    return c;
  }
  // the second half of the sweep stays where the kernel forms are densest: few inputs, R <= 4,
  // 64 tiles per stripe and more
  const bool dense = i >= kCases / 2;
  const int K = dense ? kKs[r.next() % 8] : r.pick(kKs);
  const int R = 1 + static_cast<int>(r.next() % (dense ? 4 : 16));
  const uint64_t S = dense ? kSs[9 + r.next() % 14] : r.pick(kSs);
  int batch = r.pick(kBatches);
  const uint64_t tps = (S + kTile - 1) / kTile;
  if (batch > 65535 && tps > 33) batch = 300;  // (keeps the record's text bounded)
  while (tps * static_cast<uint64_t>(batch) > (1u << 20) && batch > 1) batch /= 2;
  c.a = shape(K, R, S, batch);
  c.a.addr_tz = r.pick(kTzs);
  c.a.stripe_stride = r.pick(kStrides);
  const auto& mis = kMis[!r.one_in(dense ? 4 : 2) ? 0 : r.next() % 6];
  c.a.in_misalign = mis[0];
  c.a.out_misalign = mis[1];
  c.a.verify_mask = verify_mask(r, R, r.one_in(2) ? 0 : static_cast<int>(r.next() % 4));
  c.bytes_only = r.one_in(16);
  c.bs = static_cast<int>(r.next() % 4) % 3;
  c.mode = r.one_in(4) ? (r.one_in(2) ? 0 : 2) : 1;
  c.events = r.one_in(2);
  if (r.one_in(64)) c.a.ltabs = nullptr;
  return c;
}

std::string describe(const Case& c) {
  char b[256];
  std::snprintf(b, sizeof b, "K%d R%d S%llu b%d tz%d st%llu mis%u,%u vm%x bo%d bs%d,%d ev%d lt%d",
                c.a.K, c.a.R, static_cast<unsigned long long>(c.a.S), c.a.batch, c.a.addr_tz,
                static_cast<unsigned long long>(c.a.stripe_stride), c.a.in_misalign, c.a.out_misalign,
                c.a.verify_mask, c.bytes_only, c.bs, c.mode, c.events, c.a.ltabs != nullptr);
  return b;
}

void put(const char* f, ...) __attribute__((format(printf, 1, 2)));
void put(const char* f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  fake::log += buf;
}

void put_list(const char* what, const std::vector<int>& v) {
  fake::log += what;
  for (int o : v) put(" %d", o);
  fake::log += "\n";
}

// Codes between and beyond the families.
const int kInvalid[] = {7, 31, 39, 103, 255, 263, 511, 1100};

// The whole record of one case, left in fake::log. `form` = launch_form(a, -1).
void run_case(int i, int* form) {
  Case c = make_case(i);
  bs::Kernel kernel(c.a.K, c.a.R, nullptr);
  if (c.bs) c.a.bs = &kernel;
  fake::bs_ready = c.bs == 2;
  fake::bs_mode = c.mode;
  fake::log.clear();
  tune_table().reset(nullptr);
  const ApplyArgs& a = c.a;
  LaunchEvents ev;
  if (c.events) {
    ev.start = reinterpret_cast<hipEvent_t>(0x6000);
    ev.stop = reinterpret_cast<hipEvent_t>(0x7000);
  }
  put("case %d: %s\n", i, describe(c).c_str());
  const std::vector<int> cand = order_candidates(a, false), every = order_candidates(a, true);
  put_list("candidates:", cand);
  put_list("every instance:", every);
  put("bitslice_wanted=%d slice_tiles=%u\n", bitslice_wanted(a) ? 1 : 0, launch_slice_tiles(a.K + a.R));
  *form = launch_form(a, -1);
  std::vector<int> orders = {-1};
  for (int o : cand) orders.push_back(o);
  for (int o : every)
    if (std::find(orders.begin(), orders.end(), o) == orders.end()) orders.push_back(o);
  const size_t valid = orders.size();
  for (int o : kInvalid) orders.push_back(o);
  const uint32_t rows = (1u << a.R) - 1;
  for (size_t n = 0; n < orders.size(); ++n) {
    const int o = orders[n];
    // (the double-buffered G4 / G8 table of the A/B build has two members: code 255 on a launch
    // that can take them is not a defined request)
    if (o == 255 && kAbInstances && a.R <= 4 && a.K >= 6 && !(a.in_misalign | a.out_misalign) &&
        (a.verify_mask & rows) == 0)
      continue;
    put("order %d: form=%d\n apply\n", o, launch_form(a, o));
    put(" -> %d\n", static_cast<int>(launch_apply(a, nullptr, c.bytes_only, o, ev)));
    // the ceilings index their tables by the code's tile order: only offered codes are defined
    if (n >= valid || c.bytes_only) continue;
    for (int mode = 0; mode <= (kAbInstances ? 8 : 2); ++mode) {
      put(" ceiling %d\n", mode);
      put(" -> %d\n", static_cast<int>(launch_ceiling(a, nullptr, o, mode, ev)));
    }
  }
  if (i % 3 == 0) {  // what the tune table does with each offered code
    for (int o : every) {
      record_tuned(a, o);
      const int t = tuned_order(a);
      put("tuned %d: tuned_order=%d form=%d\n apply\n", o, t, launch_form(a, -1));
      put(" -> %d\n", static_cast<int>(launch_apply(a, nullptr, c.bytes_only, t, ev)));
    }
    record_tuned(a, 7);  // a code the launch does not offer
    put("tuned 7: tuned_order=%d\n", tuned_order(a));
    tune_table().reset(nullptr);
  }
  if (i % 5 == 0) {
    for (long long tiles : {2048LL, 0LL, -1LL}) {
      set_slice_tiles_for_tuning(tiles);
      put("slice tiles %lld: %u\n apply\n", tiles, launch_slice_tiles(a.K + a.R));
      put(" -> %d\n", static_cast<int>(launch_apply(a, nullptr, c.bytes_only, -1, ev)));
    }
  }
}

uint64_t fnv1a(const std::string& s) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned char ch : s) h = (h ^ ch) * 0x100000001b3ull;
  return h;
}

int time_selection() {
  fake::recording = false;
  std::vector<Case> cases;
  for (int i = 0; i < kCases; ++i) {
    Case c = make_case(i);
    c.a.bs = nullptr;
    cases.push_back(c);
  }
  std::vector<double> ns;
  for (int rep = 0; rep < 9; ++rep) {
    long n = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int pass = 0; pass < 20; ++pass)
      for (const Case& c : cases) {
        (void)launch_apply(c.a, nullptr, c.bytes_only, -1, {});
        ++n;
      }
    const auto t1 = std::chrono::steady_clock::now();
    ns.push_back(std::chrono::duration<double, std::nano>(t1 - t0).count() / static_cast<double>(n));
  }
  std::printf("ns per launch_apply, 9 repeats:");
  for (double v : ns) std::printf(" %.1f", v);
  std::sort(ns.begin(), ns.end());
  std::printf("\nmedian %.1f min %.1f max %.1f\n", ns[4], ns.front(), ns.back());
  return 0;
}

// The device symbol of the one vector kernel launch_apply dispatches for `a` in order code `o`
// with the bit-sliced kernels off ("?" when it dispatched none or more than one).
std::string dispatched(const ApplyArgs& a, int o) {
  fake::bs_mode = 0;
  fake::bs_ready = 0;
  fake::log.clear();
  tune_table().reset(nullptr);
  if (launch_apply(a, nullptr, false, o, {}) != hipSuccess) return "?";
  std::string name;
  size_t at = 0;
  while (at < fake::log.size()) {
    const size_t end = std::min(fake::log.find('\n', at), fake::log.size());
    const std::string line = fake::log.substr(at, end - at);
    at = end + 1;
    if (line.rfind("  attr ", 0) == 0 || line.rfind("  ", 0) != 0) continue;
    const std::string sym = line.substr(2, line.find(' ', 2) - 2);
    if (!name.empty() && sym != name) return "?";  // (a sliced grid repeats one symbol)
    name = sym;
  }
  return name.empty() ? "?" : name;
}

// The wide ring's instances (R 9..16 in consecutive order and in Q8), pinned and by the rule
// on both sides of its 256-tiles-per-stripe threshold: one line per launch with the symbol.
int wide_instances() {
  const struct { const char* name; int code; } kPins[] = {{"consecutive", 0}, {"q8", 3}};
  for (int R = 9; R <= kMaxRowsPerLaunch; ++R)
    for (const auto& pin : kPins)
      std::printf("wide R=%d order=%s %s\n", R, pin.name,
                  dispatched(shape(11, R, 3 * kTile + 16, 2), pin.code).c_str());
  for (int R = 9; R <= kMaxRowsPerLaunch; ++R)
    for (uint64_t tiles : {256, 255})
      std::printf("rule R=%d tiles=%llu %s\n", R, static_cast<unsigned long long>(tiles),
                  dispatched(shape(11, R, tiles * kTile, 2), -1).c_str());
  std::printf("launch_record ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  int stride = 1, full = -1;
  bool unreached = false;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--time")) return time_selection();
    if (!std::strcmp(argv[i], "--wide")) return wide_instances();
    if (!std::strcmp(argv[i], "--stride") && i + 1 < argc) stride = std::max(1, std::atoi(argv[++i]));
    if (!std::strcmp(argv[i], "--full") && i + 1 < argc) full = std::atoi(argv[++i]);
    if (!std::strcmp(argv[i], "--unreached")) unreached = true;
  }
  int form = -1;
  if (full >= 0) {
    run_case(full, &form);
    std::fputs(fake::log.c_str(), stdout);
    std::printf("launch_record ok\n");
    return 0;
  }
  for (int i = 0; i < kCases; i += stride) {
    run_case(i, &form);
    if (!unreached)
      std::printf("%d %s form=%d %016llx\n", i, describe(make_case(i)).c_str(), form,
                  static_cast<unsigned long long>(fnv1a(fake::log)));
  }
  if (unreached) {
    size_t reached = 0;
    for (const auto& kv : fake::kernels()) {
      if (kv.second) ++reached;
      else std::printf("unreached %s\n", kv.first.c_str());
    }
    std::printf("%zu of %zu registered kernels dispatched\n", reached, fake::kernels().size());
  }
  std::printf("launch_record ok\n");
  return 0;
}
