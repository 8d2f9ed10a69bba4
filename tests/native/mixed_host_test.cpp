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
  CHECK(build_mixed_tables(k, m, batch, pres.data(), t) == MixedError::kOk);
  CHECK(t.k == k && t.m == m && t.batch == batch);

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

}  // namespace

int main() {
  check_profile(10, 4, 40, 1);
  check_profile(20, 12, 24, 2);
  {  // too few shards anywhere in the batch fails the whole build
    const int k = 10, m = 4, n = 14;
    std::vector<uint8_t> pres(3 * n, 1);
    for (int i = 0; i < 5; ++i) pres[n + i] = 0;
    MixedTables t;
    CHECK(build_mixed_tables(k, m, 3, pres.data(), t) == MixedError::kTooFewShards);
    CHECK(!mixed_masks_equal(n, 3, pres.data()));
    std::vector<uint8_t> same(3 * n, 1);
    same[2] = same[n + 2] = same[2 * n + 2] = 0;
    same[5] = 7;  // nonzero = present
    CHECK(mixed_masks_equal(n, 3, same.data()));
  }
  std::printf("mixed_host_test ok\n");
  return 0;
}
