// Host-side tables of feed objects on the CPU, built with
// g++ -fsanitize=address,undefined by tests/test_native_feed.py:
//  - the rows are the compared indices ascending, then the wanted indices ascending; V is the
//    expected set ascending; a shard's feed position is its place in V, or k + its place among
//    the compared shards, and -1 for every other index;
//  - one inversion per object;
//  - every C entry equals the entry of decode_plan's row for a presence mask equal to the expected
//    set, and is nonzero (E is MDS), over seeded expected sets that include parity shards;
//  - every block of the arena, evaluated over all 256 inputs, is a bit-by-bit GF(2^8) multiply by
//    C[row][j] for an expected position and by the unit column for a compared one;
//  - every refusal, in the stated order.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "feed_tables.hpp"
#include "gf256.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// bit-by-bit multiply mod 0x11D: independent of gf256.hpp's log / exp tables
uint8_t slow_mul(uint8_t a, uint8_t b) {
  unsigned r = 0, x = a;
  for (int bit = 0; bit < 8; ++bit) {
    if ((b >> bit) & 1u) r ^= x;
    x <<= 1;
    if (x & 0x100u) x ^= 0x11Du;
  }
  return static_cast<uint8_t>(r);
}

// what gf_mul4 computes for one byte from a block of five words
uint8_t perm_mul(const uint32_t* w, unsigned x) {
  auto byte = [](uint32_t lo, uint32_t hi, unsigned e) {
    return static_cast<uint8_t>((e < 4 ? lo >> (8 * e) : hi >> (8 * (e - 4))) & 0xffu);
  };
  return static_cast<uint8_t>(byte(w[0], w[1], x & 7u) ^ byte(w[2], w[3], (x >> 3) & 7u) ^
                              byte(w[4], w[4], x >> 6));
}

struct Sets {
  std::vector<int> expect, wanted, compared;
};

struct Flags {
  std::vector<uint8_t> expect, dst, chk;
};

Flags flags_of(int n, const Sets& s) {
  Flags f;
  f.expect.assign(static_cast<size_t>(n), 0);
  f.dst = f.chk = f.expect;
  for (int i : s.expect) f.expect[static_cast<size_t>(i)] = static_cast<uint8_t>(1 + (i % 3));  // any nonzero value
  for (int i : s.wanted) f.dst[static_cast<size_t>(i)] = 7;
  for (int i : s.compared) f.chk[static_cast<size_t>(i)] = 9;
  return f;
}

// k of the n indices, seeded, `parity` of them parity shards where the profile allows; of the
// others `nw` wanted and `nc` compared, seeded as well
Sets seeded_sets(std::mt19937& rng, int k, int m, int parity, int nw, int nc) {
  std::vector<int> data(static_cast<size_t>(k)), par(static_cast<size_t>(m));
  for (int i = 0; i < k; ++i) data[static_cast<size_t>(i)] = i;
  for (int j = 0; j < m; ++j) par[static_cast<size_t>(j)] = k + j;
  std::shuffle(data.begin(), data.end(), rng);
  std::shuffle(par.begin(), par.end(), rng);
  parity = std::min(parity, std::min(k, m));
  Sets s;
  s.expect.assign(par.begin(), par.begin() + parity);
  s.expect.insert(s.expect.end(), data.begin(), data.begin() + (k - parity));
  std::vector<int> rest(par.begin() + parity, par.end());
  rest.insert(rest.end(), data.begin() + (k - parity), data.end());
  std::shuffle(rest.begin(), rest.end(), rng);
  CHECK(static_cast<int>(rest.size()) == m && nw + nc <= m);
  s.wanted.assign(rest.begin(), rest.begin() + nw);
  s.compared.assign(rest.begin() + nw, rest.begin() + nw + nc);
  std::sort(s.expect.begin(), s.expect.end());
  std::sort(s.wanted.begin(), s.wanted.end());
  std::sort(s.compared.begin(), s.compared.end());
  return s;
}

void check_object(int k, int m, const Sets& s) {
  const int n = k + m;
  const Flags f = flags_of(n, s);
  FeedTables t;
  CHECK(build_feed_tables(k, m, 8211, f.expect.data(), f.dst.data(), f.chk.data(), t) == FeedError::kOk);
  CHECK(t.k == k && t.m == m && t.inversions == 1);
  CHECK(t.expect == s.expect && t.compared == s.compared && t.wanted == s.wanted);
  std::vector<int> rows = s.compared;
  rows.insert(rows.end(), s.wanted.begin(), s.wanted.end());
  CHECK(t.rows == rows && t.R() == static_cast<int>(rows.size()));
  CHECK(t.positions() == k + static_cast<int>(s.compared.size()));
  CHECK(t.block_words() == rows.size() * 5);
  CHECK(t.arena.size() == static_cast<size_t>(t.positions()) * t.block_words());
  // positions: V[j] at j, compared shard c at k + c, nothing else anywhere
  for (int i = 0; i < n; ++i) {
    const auto e = std::find(s.expect.begin(), s.expect.end(), i);
    const auto c = std::find(s.compared.begin(), s.compared.end(), i);
    const int want = e != s.expect.end()     ? static_cast<int>(e - s.expect.begin())
                     : c != s.compared.end() ? k + static_cast<int>(c - s.compared.begin())
                                             : -1;
    CHECK(t.position(i) == want);
  }
  CHECK(t.position(-1) == -1 && t.position(n) == -1);
  // C against decode_plan with every shard outside the expected set missing
  std::vector<uint8_t> present(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) present[static_cast<size_t>(i)] = f.expect[static_cast<size_t>(i)] != 0;
  DecodePlan dp;
  CHECK(decode_plan(k, m, present.data(), dp));
  CHECK(dp.valid == s.expect && dp.check.empty());
  CHECK(t.C.rows == t.R() && t.C.cols == k);
  for (int r = 0; r < t.R(); ++r) {
    const auto at = std::find(dp.missing.begin(), dp.missing.end(), rows[static_cast<size_t>(r)]);
    CHECK(at != dp.missing.end());
    for (int j = 0; j < k; ++j) {
      CHECK(t.C.at(r, j) == dp.rows.at(static_cast<int>(at - dp.missing.begin()), j));
      CHECK(t.C.at(r, j) != 0);
    }
  }
  // every block word, over all 256 inputs
  for (int p = 0; p < t.positions(); ++p)
    for (int r = 0; r < t.R(); ++r) {
      const uint8_t c = p < k ? t.C.at(r, p) : static_cast<uint8_t>(rows[static_cast<size_t>(r)] == s.compared[static_cast<size_t>(p - k)]);
      if (p >= k) CHECK((c == 1) == (r == p - k));  // a compared shard's own row is its number
      const uint32_t* w = &t.arena[static_cast<size_t>(p) * t.block_words() + static_cast<size_t>(r) * 5];
      for (unsigned x = 0; x < 256; ++x) CHECK(perm_mul(w, x) == slow_mul(c, static_cast<uint8_t>(x)));
      CHECK((w[0] == 0) == (c == 0));  // what the merge kernel reads to skip a row
    }
}

void check_refusals() {
  const int k = 4, m = 3, n = 7;
  FeedTables t;
  auto build = [&](const Sets& s, size_t S) {
    const Flags f = flags_of(n, s);
    return build_feed_tables(k, m, S, f.expect.data(), f.dst.data(), f.chk.data(), t);
  };
  const std::vector<int> V = {0, 2, 3, 5};
  CHECK(build({V, {1}, {4, 6}}, 1) == FeedError::kOk);
  CHECK(build({V, {}, {}}, 1) == FeedError::kOk && t.R() == 0 && t.arena.empty());
  // the expect count, before a misplaced pointer, the row count and a zero size
  CHECK(build({{0, 2, 3}, {0}, {0}}, 0) == FeedError::kTooFewShards);
  CHECK(build({{0, 1, 2, 3, 5}, {0}, {0}}, 0) == FeedError::kArg);
  // a misplaced pointer, before a zero size
  CHECK(build({V, {0}, {}}, 0) == FeedError::kArg);      // a dst at an expected index
  CHECK(build({V, {}, {5}}, 0) == FeedError::kArg);      // a check at an expected index
  CHECK(build({V, {1, 4}, {4}}, 0) == FeedError::kArg);  // a check and a dst at one index
  // a zero size
  CHECK(build({V, {1}, {4, 6}}, 0) == FeedError::kNoData);
  CHECK(build({V, {}, {}}, 0) == FeedError::kNoData);
  // RS(10,20): 16 rows build, 17 are refused -- after a misplaced pointer, before a zero size
  std::vector<int> e10, rows16, rows17;
  for (int i = 0; i < 10; ++i) e10.push_back(i);
  for (int i = 10; i < 26; ++i) rows16.push_back(i);
  rows17 = rows16;
  rows17.push_back(26);
  auto build30 = [&](const std::vector<int>& wanted, const std::vector<int>& compared, size_t S) {
    const Flags f = flags_of(30, {e10, wanted, compared});
    return build_feed_tables(10, 20, S, f.expect.data(), f.dst.data(), f.chk.data(), t);
  };
  CHECK(build30(rows16, {}, 40) == FeedError::kOk && t.R() == 16);
  CHECK(build30({}, rows16, 40) == FeedError::kOk && t.R() == 16 && t.positions() == 26);
  CHECK(build30(rows17, {}, 0) == FeedError::kUnsupported);
  CHECK(build30({10, 11, 12, 13, 14, 15, 16, 17, 18}, {19, 20, 21, 22, 23, 24, 25, 26}, 0) == FeedError::kUnsupported);
  CHECK(build30(rows17, {3}, 0) == FeedError::kArg);
}

}  // namespace

int main() {
  std::mt19937 rng(20251);
  const int profiles[][2] = {{10, 4}, {4, 2}, {3, 2}, {1, 3}, {16, 4}, {10, 8}, {20, 12}};
  for (const auto& pr : profiles) {
    const int k = pr[0], m = pr[1];
    for (int parity = 0; parity <= std::min(k, m); ++parity)
      for (int nw = 0; nw <= m - parity; ++nw)
        for (int nc = 0; nw + nc <= m - parity; nc += (m > 6 ? 3 : 1))
          check_object(k, m, seeded_sets(rng, k, m, parity, nw, nc));
    // all m rows wanted, all compared, and the split the session tests use
    check_object(k, m, seeded_sets(rng, k, m, 0, m, 0));
    check_object(k, m, seeded_sets(rng, k, m, 0, 0, m));
    check_object(k, m, seeded_sets(rng, k, m, 0, 1, m - 1));
  }
  check_refusals();
  std::printf("feed_tables_test ok\n");
  return 0;
}
