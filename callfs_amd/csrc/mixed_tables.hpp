// Host-side tables of a mixed device plan (rs_plan_create_mixed): a batch
// in which every stripe has its own presence mask. The batch's masks are deduplicated
// into P distinct patterns; every pattern of RS(k,m) has exactly m rows (its missing
// shards are written, its present shards beyond the first k are compared), so all
// patterns share one launch-group structure: groups of up to 16 rows, and per group one
// arena that holds every pattern's nibble tables back to back. Plain C++ with no HIP
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
  std::vector<int> rows;      // m shard indices: the missing ones, then the compared ones
  int missing = 0;            // rows[0 .. missing) are written, the rest compared
};

// One launch group: rows [row0, row0 + R) of every pattern.
struct MixedGroup {
  int row0 = 0;
  int R = 0;
  size_t tab_stride = 0;        // bytes of one pattern's tables: k * 32 * nibble_width(R)
  std::vector<uint8_t> arena;   // [P][k][32][W]: pattern p's tables at p * tab_stride
  std::vector<uint32_t> vmask;  // [P]: bit r set = row row0 + r of pattern p is compared
  // build_mixed_tables_required only (else empty): [P] rows of pattern p inside this group,
  // 0..R; table columns at and past nrows[p] are zero
  std::vector<uint32_t> nrows;
};

struct MixedTables {
  int k = 0, m = 0, batch = 0;
  int rows = 0;  // rows of every pattern: m, or the missing count of build_mixed_tables_missing
  std::vector<MixedPattern> patterns;  // P distinct masks, in order of first appearance
  std::vector<uint32_t> pat;           // [batch]: stripe b's pattern
  std::vector<MixedGroup> groups;
  int P() const { return static_cast<int>(patterns.size()); }
};

enum class MixedError { kOk, kTooFewShards, kSingular, kRowCount };

// The builder behind both forms below. rows == m: every pattern's m rows, missing then
// compared. rows < m or missing_only: the e = rows missing shards alone (all written); a
// stripe with another missing count is reported as kRowCount.
inline MixedError build_mixed_rows(int k, int m, int rows, bool missing_only, int batch,
                                   const uint8_t* present, MixedTables& t) {
  const int n = k + m;
  t = MixedTables();
  t.k = k;
  t.m = m;
  t.rows = rows;
  t.batch = batch;
  t.pat.resize(static_cast<size_t>(batch));
  std::map<std::string, uint32_t> seen;
  std::vector<DecodePlan> plans;
  for (int b = 0; b < batch; ++b) {
    std::string key(static_cast<size_t>(n), '0');
    int np = 0;
    for (int i = 0; i < n; ++i)
      if (present[static_cast<size_t>(b) * n + i]) {
        key[static_cast<size_t>(i)] = '1';
        ++np;
      }
    if (np < k) return MixedError::kTooFewShards;
    auto it = seen.find(key);
    if (it == seen.end()) {
      MixedPattern p;
      p.mask.resize(static_cast<size_t>(n));
      for (int i = 0; i < n; ++i) p.mask[static_cast<size_t>(i)] = key[static_cast<size_t>(i)] == '1';
      DecodePlan dp;
      if (!decode_plan(k, m, p.mask.data(), dp)) return MixedError::kSingular;
      p.valid = dp.valid;
      p.rows = dp.missing;
      p.missing = static_cast<int>(dp.missing.size());
      if (missing_only) {
        if (p.missing != rows) return MixedError::kRowCount;
      } else {
        p.rows.insert(p.rows.end(), dp.check.begin(), dp.check.end());
      }
      it = seen.emplace(key, static_cast<uint32_t>(t.patterns.size())).first;
      t.patterns.push_back(std::move(p));
      plans.push_back(std::move(dp));
    }
    t.pat[static_cast<size_t>(b)] = it->second;
  }
  const size_t P = t.patterns.size();
  for (int g0 = 0; g0 < rows; g0 += kMixedRowsPerLaunch) {
    MixedGroup g;
    g.row0 = g0;
    g.R = std::min(kMixedRowsPerLaunch, rows - g0);
    const size_t per_shard = 32u * static_cast<size_t>(nibble_width(g.R));
    g.tab_stride = static_cast<size_t>(k) * per_shard;
    g.arena.assign(P * g.tab_stride, 0);
    g.vmask.assign(P, 0);
    for (size_t p = 0; p < P; ++p) {
      const MixedPattern& pt = t.patterns[p];
      for (int r = 0; r < g.R; ++r)
        if (g0 + r >= pt.missing) g.vmask[p] |= 1u << r;
      for (int i = 0; i < k; ++i) {
        uint8_t col[kMixedRowsPerLaunch] = {0};
        for (int r = 0; r < g.R; ++r) col[r] = plans[p].rows.at(g0 + r, i);
        nibble_tables(col, g.R, &g.arena[p * g.tab_stride + static_cast<size_t>(i) * per_shard]);
      }
    }
    t.groups.push_back(std::move(g));
  }
  return MixedError::kOk;
}

// present: batch * (k + m) flags, stripe b's mask at present + b * (k + m); nonzero =
// present. Fills `t`; on an error `t` is left in an unspecified state.
inline MixedError build_mixed_tables(int k, int m, int batch, const uint8_t* present,
                                     MixedTables& t) {
  return build_mixed_rows(k, m, m, false, batch, present, t);
}

// The form for reconstructs without verification (the host path's ragged batches): every
// stripe of the batch has exactly e missing shards (1 <= e <= m), a pattern's rows are those
// alone, all written, and the launch groups are cut over e instead of m.
inline MixedError build_mixed_tables_missing(int k, int m, int e, int batch,
                                             const uint8_t* present, MixedTables& t) {
  return build_mixed_rows(k, m, e, true, batch, present, t);
}

// The form for ReconstructSome (rs_plan_create_required): required holds
// batch * (k + m) flags beside present's, and a missing shard whose flag is clear has no row
// (it is neither written nor read); flags on present shards are ignored. Patterns are
// distinct (mask, wanted missing shards) pairs, so pattern p has its own row count
// r_p = patterns[p].rows.size() <= m: its written rows (patterns[p].missing of them), then its
// compared rows. t.rows is the largest r_p, the launch groups are cut over it, and group g
// holds in nrows[p] how many of pattern p's rows fall inside it (0 when r_p <= g.row0).
// vmask as in every form. with_check = false (a reconstruct without verification) drops the
// compared rows: a pattern's rows are its wanted missing shards alone.
inline MixedError build_mixed_tables_required(int k, int m, int batch, const uint8_t* present,
                                              const uint8_t* required, MixedTables& t,
                                              bool with_check = true) {
  const int n = k + m;
  t = MixedTables();
  t.k = k;
  t.m = m;
  t.batch = batch;
  t.pat.resize(static_cast<size_t>(batch));
  std::map<std::string, uint32_t> seen;
  std::vector<DecodePlan> plans;
  std::vector<uint8_t> wanted(static_cast<size_t>(n));
  for (int b = 0; b < batch; ++b) {
    const uint8_t* pr = present + static_cast<size_t>(b) * n;
    const uint8_t* rq = required + static_cast<size_t>(b) * n;
    // '1' present, 'w' missing and wanted, '0' missing and not wanted
    std::string key(static_cast<size_t>(n), '0');
    int np = 0;
    for (int i = 0; i < n; ++i) {
      if (pr[i]) {
        key[static_cast<size_t>(i)] = '1';
        ++np;
      } else if (rq[i]) {
        key[static_cast<size_t>(i)] = 'w';
      }
    }
    if (np < k) return MixedError::kTooFewShards;
    auto it = seen.find(key);
    if (it == seen.end()) {
      MixedPattern p;
      p.mask.resize(static_cast<size_t>(n));
      for (int i = 0; i < n; ++i) {
        p.mask[static_cast<size_t>(i)] = key[static_cast<size_t>(i)] == '1';
        wanted[static_cast<size_t>(i)] = key[static_cast<size_t>(i)] == 'w';
      }
      DecodePlan dp;
      if (!decode_plan(k, m, p.mask.data(), wanted.data(), dp)) return MixedError::kSingular;
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
  return MixedError::kOk;
}

// True when every missing shard of every stripe is wanted (required null counts as that).
inline bool required_all_wanted(int n, int batch, const uint8_t* present, const uint8_t* required) {
  if (!required) return true;
  for (size_t j = 0; j < static_cast<size_t>(batch) * n; ++j)
    if (!present[j] && !required[j]) return false;
  return true;
}

// True when every stripe has the same (mask, wanted missing shards) pair.
inline bool required_pairs_equal(int n, int batch, const uint8_t* present, const uint8_t* required) {
  for (int b = 1; b < batch; ++b)
    for (int i = 0; i < n; ++i) {
      const size_t j = static_cast<size_t>(b) * n + i;
      if ((present[j] != 0) != (present[i] != 0)) return false;
      if (!present[i] && (required[j] != 0) != (required[i] != 0)) return false;
    }
  return true;
}

// True when every stripe of the batch has the same mask (as 0 / nonzero flags).
inline bool mixed_masks_equal(int n, int batch, const uint8_t* present) {
  for (int b = 1; b < batch; ++b)
    for (int i = 0; i < n; ++i)
      if ((present[static_cast<size_t>(b) * n + i] != 0) != (present[i] != 0)) return false;
  return true;
}

}  // namespace callfs
