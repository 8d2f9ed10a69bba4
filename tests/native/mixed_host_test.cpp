// Host-side tables of mixed device plans (callfs_amd/csrc/mixed_tables.hpp) on the CPU,
// built with g++ -fsanitize=address,undefined by tests/test_native_mixed.py.
// For seeded batches of per-stripe presence masks: the masks deduplicate into the distinct
// patterns, every pattern's arena slice is nibble_tables of its decode_plan rows, vmask
// marks exactly the compared rows, and a byte-wise evaluation of the arena tables (what the
// kernels do per byte) reproduces every stripe's missing shards and agrees with its compared
// ones.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "gf256.hpp"
#include "mixed_tables.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// batch masks with 0..m losses each; a few stripes repeat earlier masks
std::vector<uint8_t> seeded_masks(int k, int m, int batch, unsigned seed) {
  const int n = k + m;
  std::mt19937 rng(seed);
  std::vector<uint8_t> pres(static_cast<size_t>(batch) * n, 1);
  for (int b = 0; b < batch; ++b) {
    uint8_t* row = &pres[static_cast<size_t>(b) * n];
    if (b >= 4 && b % 5 == 4) {  // a repeat of an earlier stripe's mask
      const int src = static_cast<int>(rng() % static_cast<unsigned>(b));
      std::copy(&pres[static_cast<size_t>(src) * n], &pres[static_cast<size_t>(src) * n] + n, row);
      continue;
    }
    const int losses = static_cast<int>(rng() % static_cast<unsigned>(m + 1));
    for (int l = 0; l < losses;) {
      const int i = static_cast<int>(rng() % static_cast<unsigned>(n));
      if (row[i]) {
        row[i] = 0;
        ++l;
      }
    }
    if (b == 1)  // any nonzero byte counts as present
      for (int i = 0; i < n; ++i) row[i] = row[i] ? 0x80 : 0;
  }
  return pres;
}

void check_profile(int k, int m, int batch, unsigned seed) {
  const int n = k + m;
  const size_t S = 37;
  const std::vector<uint8_t> pres = seeded_masks(k, m, batch, seed);
  MixedTables t;
  CHECK(build_mixed_tables(k, m, batch, pres.data(), nullptr, t) == TableError::kOk);
  CHECK(t.k == k && t.m == m && t.batch == batch);
  CHECK(t.rows == m && t.uniform_rows && mixed_rows_are(t, m) && !mixed_rows_are(t, m - 1));

  // deduplication: P = number of distinct masks, pat[b] points at an equal mask
  std::set<std::string> distinct;
  for (int b = 0; b < batch; ++b) {
    std::string key;
    for (int i = 0; i < n; ++i) key.push_back(pres[static_cast<size_t>(b) * n + i] ? '1' : '0');
    distinct.insert(key);
  }
  CHECK(static_cast<size_t>(t.P()) == distinct.size());
  CHECK(t.pat.size() == static_cast<size_t>(batch));
  for (int b = 0; b < batch; ++b) {
    CHECK(t.pat[b] < static_cast<uint32_t>(t.P()));
    const MixedPattern& p = t.patterns[t.pat[b]];
    CHECK(p.mask.size() == static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) CHECK((p.mask[i] != 0) == (pres[static_cast<size_t>(b) * n + i] != 0));
  }
  for (int p = 0; p < t.P(); ++p)
    for (int q = p + 1; q < t.P(); ++q) CHECK(t.patterns[p].mask != t.patterns[q].mask);

  // the launch groups: m rows in groups of up to 16, the same for every pattern
  int rows = 0;
  for (const MixedGroup& g : t.groups) {
    CHECK(g.row0 == rows && g.R >= 1 && g.R <= kMixedRowsPerLaunch);
    CHECK(g.tab_stride == static_cast<size_t>(k) * 32u * nibble_width(g.R));
    CHECK(g.tab_stride % 256 == 0);
    CHECK(g.arena.size() == static_cast<size_t>(t.P()) * g.tab_stride);
    CHECK(g.vmask.size() == static_cast<size_t>(t.P()));
    CHECK(g.nrows == std::vector<uint32_t>(static_cast<size_t>(t.P()), static_cast<uint32_t>(g.R)));
    rows += g.R;
  }
  CHECK(rows == m);
  CHECK(t.groups.size() == static_cast<size_t>((m + kMixedRowsPerLaunch - 1) / kMixedRowsPerLaunch));

  // every pattern: its rows, its arena slices and its compare masks against decode_plan
  for (int p = 0; p < t.P(); ++p) {
    const MixedPattern& pt = t.patterns[p];
    DecodePlan dp;
    CHECK(decode_plan(k, m, pt.mask.data(), dp));
    CHECK(pt.valid == dp.valid);
    CHECK(pt.missing == static_cast<int>(dp.missing.size()));
    CHECK(pt.rows.size() == static_cast<size_t>(m));
    for (size_t r = 0; r < dp.missing.size(); ++r) CHECK(pt.rows[r] == dp.missing[r]);
    for (size_t r = 0; r < dp.check.size(); ++r) CHECK(pt.rows[dp.missing.size() + r] == dp.check[r]);
    for (const MixedGroup& g : t.groups) {
      const size_t per_shard = 32u * static_cast<size_t>(nibble_width(g.R));
      std::vector<uint8_t> want(per_shard);
      for (int i = 0; i < k; ++i) {
        uint8_t col[kMixedRowsPerLaunch] = {0};
        for (int r = 0; r < g.R; ++r) col[r] = dp.rows.at(g.row0 + r, i);
        nibble_tables(col, g.R, want.data());
        CHECK(std::equal(want.begin(), want.end(),
                         g.arena.begin() + static_cast<long>(p * g.tab_stride + i * per_shard)));
      }
      uint32_t vm = 0;
      for (int r = 0; r < g.R; ++r)
        if (g.row0 + r >= static_cast<int>(dp.missing.size())) vm |= 1u << r;
      CHECK(g.vmask[p] == vm);
    }
  }

  // consistent stripes; every row of every stripe evaluated byte by byte from the arena
  Mat E;
  CHECK(encode_matrix(k, m, E));
  const GF& g8 = gf();
  std::mt19937 rng(seed ^ 0x5eedu);
  for (int b = 0; b < batch; ++b) {
    std::vector<std::vector<uint8_t>> sh(n, std::vector<uint8_t>(S));
    for (int i = 0; i < k; ++i)
      for (size_t x = 0; x < S; ++x) sh[i][x] = static_cast<uint8_t>(rng());
    for (int j = k; j < n; ++j)
      for (size_t x = 0; x < S; ++x) {
        uint8_t v = 0;
        for (int i = 0; i < k; ++i) v ^= g8.mul[E.at(j, i)][sh[i][x]];
        sh[j][x] = v;
      }
    const uint32_t p = t.pat[b];
    const MixedPattern& pt = t.patterns[p];
    for (const MixedGroup& g : t.groups) {
      const int W = nibble_width(g.R);
      const uint8_t* tabs = &g.arena[p * g.tab_stride];
      for (int r = 0; r < g.R; ++r) {
        const std::vector<uint8_t>& want = sh[pt.rows[g.row0 + r]];
        for (size_t x = 0; x < S; ++x) {
          uint8_t v = 0;
          for (int i = 0; i < k; ++i) {
            const uint8_t in = sh[pt.valid[i]][x];
            const uint8_t* ti = tabs + static_cast<size_t>(i) * 32u * W;
            v ^= ti[(in & 15) * W + r] ^ ti[(16 + (in >> 4)) * W + r];
          }
          CHECK(v == want[x]);
        }
      }
    }
  }
  std::printf("RS(%d,%d) batch %d: %d patterns, %zu launch group(s) ok\n", k, m, batch, t.P(),
              t.groups.size());
}

// every field of two tables, byte for byte
void check_same(const MixedTables& a, const MixedTables& b) {
  CHECK(a.k == b.k && a.m == b.m && a.batch == b.batch && a.rows == b.rows);
  CHECK(a.uniform_rows == b.uniform_rows && a.pat == b.pat && a.P() == b.P());
  for (int p = 0; p < a.P(); ++p) {
    CHECK(a.patterns[p].mask == b.patterns[p].mask && a.patterns[p].valid == b.patterns[p].valid);
    CHECK(a.patterns[p].rows == b.patterns[p].rows && a.patterns[p].missing == b.patterns[p].missing);
  }
  CHECK(a.groups.size() == b.groups.size());
  for (size_t g = 0; g < a.groups.size(); ++g) {
    CHECK(a.groups[g].row0 == b.groups[g].row0 && a.groups[g].R == b.groups[g].R);
    CHECK(a.groups[g].tab_stride == b.groups[g].tab_stride && a.groups[g].arena == b.groups[g].arena);
    CHECK(a.groups[g].vmask == b.groups[g].vmask && a.groups[g].nrows == b.groups[g].nrows);
  }
}

// The full reconstruct is the all-wanted case of the one builder: a null wanted set, every
// missing shard flagged, and every shard flagged (flags on present shards count for nothing)
// give the same tables, with and without the compared rows.
void builder_identity(int k, int m, const std::vector<uint8_t>& pres) {
  const int n = k + m, batch = static_cast<int>(pres.size()) / n;
  std::vector<uint8_t> missing(pres.size()), ones(pres.size(), 1);
  for (size_t j = 0; j < pres.size(); ++j) missing[j] = !pres[j];
  for (bool with_check : {true, false}) {
    MixedTables null, flagged, all;
    CHECK(build_mixed_tables(k, m, batch, pres.data(), nullptr, null, with_check) == TableError::kOk);
    CHECK(build_mixed_tables(k, m, batch, pres.data(), missing.data(), flagged, with_check) == TableError::kOk);
    CHECK(build_mixed_tables(k, m, batch, pres.data(), ones.data(), all, with_check) == TableError::kOk);
    check_same(null, flagged);
    check_same(null, all);
    int max_rows = 0;
    for (const MixedPattern& pt : null.patterns) {
      DecodePlan dp;
      CHECK(decode_plan(k, m, pt.mask.data(), dp));
      CHECK(pt.rows.size() == dp.missing.size() + (with_check ? dp.check.size() : 0));
      max_rows = std::max(max_rows, static_cast<int>(pt.rows.size()));
    }
    CHECK(null.rows == max_rows);
    if (!with_check) continue;
    // every pattern has m rows: nrows is R in every group (the last group's R is the remainder)
    CHECK(null.rows == m && null.uniform_rows);
    CHECK(null.groups.size() == static_cast<size_t>((m + kMixedRowsPerLaunch - 1) / kMixedRowsPerLaunch));
    for (const MixedGroup& g : null.groups)
      for (uint32_t nr : g.nrows) CHECK(nr == static_cast<uint32_t>(g.R));
  }
  std::printf("RS(%d,%d) batch %d: null, flagged and all-ones wanted sets build equal tables ok\n", k, m, batch);
}

}  // namespace

int main() {
  check_profile(10, 4, 40, 1);
  check_profile(20, 12, 24, 2);
  {  // RS(4,2): every mask with at least k present, in ascending and then descending order
    const int n = 6;
    std::vector<uint8_t> pres;
    for (int pass = 0; pass < 2; ++pass)
      for (unsigned i = 0; i < (1u << n); ++i) {
        const unsigned pm = pass ? (1u << n) - 1 - i : i;
        if (__builtin_popcount(pm) < 4) continue;
        for (int b = 0; b < n; ++b) pres.push_back((pm >> b) & 1u);
      }
    CHECK(pres.size() == 2u * 22 * n);
    builder_identity(4, 2, pres);
  }
  {  // RS(3,20): 16 + 4 rows, two launch groups
    const int n = 23;
    const int lost[5] = {20, 0, 7, 20, 16};  // stripe s misses shards first[s] .. first[s] + lost[s] - 1
    const int first[5] = {0, 0, 2, 3, 1};
    std::vector<uint8_t> pres(5 * n, 1);
    for (int s = 0; s < 5; ++s)
      for (int i = 0; i < lost[s]; ++i) pres[s * n + first[s] + i] = 0;
    builder_identity(3, 20, pres);
  }
  {  // too few shards anywhere in the batch fails the whole build
    const int k = 10, m = 4, n = 14;
    std::vector<uint8_t> pres(3 * n, 1);
    for (int i = 0; i < 5; ++i) pres[n + i] = 0;
    MixedTables t;
    CHECK(build_mixed_tables(k, m, 3, pres.data(), nullptr, t) == TableError::kTooFewShards);
    CHECK(!required_pairs_equal(n, 3, pres.data(), nullptr));
    std::vector<uint8_t> same(3 * n, 1);
    same[2] = same[n + 2] = same[2 * n + 2] = 0;
    same[5] = 7;  // nonzero = present
    CHECK(required_pairs_equal(n, 3, same.data(), nullptr));
  }
  std::printf("mixed_host_test ok\n");
  return 0;
}
