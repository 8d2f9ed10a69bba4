// Host-side tables of a mixed device plan (rs_plan_create_mixed): a batch
// in which every stripe has its own presence mask and, for ReconstructSome (§5.10), its own
// set of wanted missing shards. The batch's (mask, wanted) pairs are deduplicated into P
// distinct patterns; pattern p has r_p <= m rows (its wanted missing shards are written, its
// present shards beyond the first k are compared). The launch groups are cut over the largest
// r_p in steps of up to 16 rows, and per group one arena holds every pattern's nibble tables
// back to back. With every missing shard wanted each pattern of RS(k,m) has exactly m rows:
// the full reconstruct is the all-wanted case of the one builder. Plain C++ with no HIP
// dependence: tests/native/mixed_host_test.cpp builds it with g++ on the CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "gf256.hpp"

namespace callfs {

constexpr int kMixedRowsPerLaunch = 16;  // rs_kernels.hpp kMaxRowsPerLaunch

struct MixedPattern {
  std::vector<uint8_t> mask;  // n flags (0 / 1)
  std::vector<int> valid;     // the k shard indices read: the first k present
  std::vector<int> rows;      // r_p shard indices: the wanted missing ones, then the compared ones
  int missing = 0;            // rows[0 .. missing) are written, the rest compared
};

// One launch group: rows [row0, row0 + R) of every pattern.
struct MixedGroup {
  int row0 = 0;
  int R = 0;
  size_t tab_stride = 0;        // bytes of one pattern's tables: k * 32 * nibble_width(R)
  std::vector<uint8_t> arena;   // [P][k][32][W]: pattern p's tables at p * tab_stride
  std::vector<uint32_t> vmask;  // [P]: bit r set = row row0 + r of pattern p is compared
  // [P] rows of pattern p inside this group, 0..R (R wherever every pattern has the same row
  // count, but for the last group's remainder); table columns at and past nrows[p] are zero
  std::vector<uint32_t> nrows;
};

struct MixedTables {
  int k = 0, m = 0, batch = 0;
  int rows = 0;               // the largest row count of a pattern: the launch groups cover it
  bool uniform_rows = true;   // every pattern has exactly `rows` rows
  std::vector<MixedPattern> patterns;  // P distinct masks, in order of first appearance
  std::vector<uint32_t> pat;           // [batch]: stripe b's pattern
  std::vector<MixedGroup> groups;
  int P() const { return static_cast<int>(patterns.size()); }
};

// What building a plan's tables can report; kNoData (a zero shard size) and kTooManyTiles are
// ragged_tables.hpp's.
enum class TableError { kOk, kNoData, kTooManyTiles, kTooFewShards, kSingular };

// present: batch * (k + m) flags, stripe b's mask at present + b * (k + m); nonzero = present.
// wanted: as many flags beside them, or null for "every missing shard": a missing shard whose
// flag is clear has no row (it is neither written nor read); flags on present shards are
// ignored. Patterns are the distinct (mask, wanted missing shards) pairs in order of first
// appearance. Pattern p's rows are its written rows (patterns[p].missing of them), then, with
// with_check, its compared rows; t.rows is the largest row count, the launch groups are cut
// over it, and group g holds in nrows[p] how many of pattern p's rows fall inside it (0 when
// r_p <= g.row0). with_check = false (a reconstruct without verification) drops the compared
// rows. Fills `t`; on an error `t` is left in an unspecified state.
inline TableError build_mixed_tables(int k, int m, int batch, const uint8_t* present,
                                     const uint8_t* wanted, MixedTables& t, bool with_check = true) {
  const int n = k + m;
  t = MixedTables();
  t.k = k;
  t.m = m;
  t.batch = batch;
  t.pat.resize(static_cast<size_t>(batch));
  std::map<std::string, uint32_t> seen;
  std::vector<DecodePlan> plans;
  std::vector<uint8_t> want(static_cast<size_t>(n));
  for (int b = 0; b < batch; ++b) {
    const size_t at = static_cast<size_t>(b) * n;
    // '1' present, 'w' missing and wanted, '0' missing and not wanted
    std::string key(static_cast<size_t>(n), '0');
    int np = 0;
    for (int i = 0; i < n; ++i) {
      if (present[at + i]) {
        key[static_cast<size_t>(i)] = '1';
        ++np;
      } else if (!wanted || wanted[at + i]) {
        key[static_cast<size_t>(i)] = 'w';
      }
    }
    if (np < k) return TableError::kTooFewShards;
    auto it = seen.find(key);
    if (it == seen.end()) {
      MixedPattern p;
      p.mask.resize(static_cast<size_t>(n));
      for (int i = 0; i < n; ++i) {
        p.mask[static_cast<size_t>(i)] = key[static_cast<size_t>(i)] == '1';
        want[static_cast<size_t>(i)] = key[static_cast<size_t>(i)] == 'w';
      }
      DecodePlan dp;
      if (!decode_plan(k, m, p.mask.data(), want.data(), dp)) return TableError::kSingular;
      p.valid = dp.valid;
      p.rows = dp.missing;
      p.missing = static_cast<int>(dp.missing.size());
      if (with_check) p.rows.insert(p.rows.end(), dp.check.begin(), dp.check.end());
      t.rows = std::max(t.rows, static_cast<int>(p.rows.size()));
      it = seen.emplace(key, static_cast<uint32_t>(t.patterns.size())).first;
      t.patterns.push_back(std::move(p));
      plans.push_back(std::move(dp));
    }
    t.pat[static_cast<size_t>(b)] = it->second;
  }
  for (const MixedPattern& pt : t.patterns)
    t.uniform_rows &= static_cast<int>(pt.rows.size()) == t.rows;
  const size_t P = t.patterns.size();
  for (int g0 = 0; g0 < t.rows; g0 += kMixedRowsPerLaunch) {
    MixedGroup g;
    g.row0 = g0;
    g.R = std::min(kMixedRowsPerLaunch, t.rows - g0);
    const size_t per_shard = 32u * static_cast<size_t>(nibble_width(g.R));
    g.tab_stride = static_cast<size_t>(k) * per_shard;
    g.arena.assign(P * g.tab_stride, 0);
    g.vmask.assign(P, 0);
    g.nrows.assign(P, 0);
    for (size_t p = 0; p < P; ++p) {
      const MixedPattern& pt = t.patterns[p];
      const int rp = static_cast<int>(pt.rows.size());
      const int nr = std::max(0, std::min(g.R, rp - g0));
      g.nrows[p] = static_cast<uint32_t>(nr);
      for (int r = 0; r < nr; ++r)
        if (g0 + r >= pt.missing) g.vmask[p] |= 1u << r;
      if (nr == 0) continue;
      for (int i = 0; i < k; ++i) {
        uint8_t col[kMixedRowsPerLaunch] = {0};
        for (int r = 0; r < nr; ++r) col[r] = plans[p].rows.at(g0 + r, i);
        nibble_tables(col, g.R, &g.arena[p * g.tab_stride + static_cast<size_t>(i) * per_shard]);
      }
    }
    t.groups.push_back(std::move(g));
  }
  return TableError::kOk;
}

// What the mixed and ragged kernels rest on (they have no per-pattern row count): every pattern
// has exactly `rows` rows. The host path's classes (ragged_chunks.hpp) are cut so that it holds.
inline bool mixed_rows_are(const MixedTables& t, int rows) { return t.uniform_rows && t.rows == rows; }

// True when every missing shard of every stripe is wanted (required null counts as that).
inline bool required_all_wanted(int n, int batch, const uint8_t* present, const uint8_t* required) {
  if (!required) return true;
  for (size_t j = 0; j < static_cast<size_t>(batch) * n; ++j)
    if (!present[j] && !required[j]) return false;
  return true;
}

// True when every stripe has the same (mask, wanted missing shards) pair; masks as 0 / nonzero
// flags, required null = every missing shard wanted, so the masks alone are compared.
inline bool required_pairs_equal(int n, int batch, const uint8_t* present, const uint8_t* required) {
  for (int b = 1; b < batch; ++b)
    for (int i = 0; i < n; ++i) {
      const size_t j = static_cast<size_t>(b) * n + i;
      if ((present[j] != 0) != (present[i] != 0)) return false;
      if (required && !present[i] && (required[j] != 0) != (required[i] != 0)) return false;
    }
  return true;
}

}  // namespace callfs
