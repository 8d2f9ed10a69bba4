// Host-side tables of a feed object (rs_feed_create): one stripe whose k expected
// shards, wanted shards and compared shards are fixed up front and whose shards are then
// delivered one per launch. With V the expected indices in ascending order, the rows are the
// compared indices ascending, then the wanted indices ascending (a decode-repair plan's order),
// and C = E[rows] . inv(E[V]) comes from one decode_plan call: one k x k inversion per object.
// A shard is delivered at its feed position: V[j] at position j, compared shard number c (in
// ascending order) at position k + c. Per position the arena holds one block of `rows` x 5 words,
// the v_perm tables (gf256.hpp perm_tables) of the position's column: C[.][j] for an expected
// position, the unit column (1 in the shard's own row, 0 elsewhere) for a compared one. A launch
// picks its block by position; nothing is built after create. Plain C++ with no HIP dependence:
// tests/native/feed_tables_test.cpp builds it with g++ on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "gf256.hpp"

namespace callfs {

constexpr int kFeedMaxRows = 16;

// What build_feed_tables refuses, in the order it checks: the expected count (fewer than k:
// kTooFewShards, more: kArg), then the misplaced pointers (a dst or a check at an expected index,
// a dst and a check at one index: kArg), then more than kFeedMaxRows rows (kUnsupported), then a
// zero size (kNoData); kSingular cannot happen for k + m <= 256.
enum class FeedError { kOk, kArg, kTooFewShards, kUnsupported, kNoData, kSingular };

struct FeedTables {
  int k = 0, m = 0;
  int inversions = 0;         // k x k inversions done for this object
  std::vector<int> expect;    // V: k indices, ascending
  std::vector<int> compared;  // ascending
  std::vector<int> wanted;    // ascending
  std::vector<int> rows;      // compared, then wanted
  Mat C;                      // rows x k, column j for V[j]
  std::vector<uint32_t> arena;  // [positions()][R()][kTabWords]
  int R() const { return static_cast<int>(rows.size()); }
  int positions() const { return k + static_cast<int>(compared.size()); }
  size_t block_words() const { return rows.size() * kTabWords; }
  // the feed position of shard idx, -1 when it is neither expected nor compared
  int position(int idx) const {
    for (size_t j = 0; j < expect.size(); ++j)
      if (expect[j] == idx) return static_cast<int>(j);
    for (size_t c = 0; c < compared.size(); ++c)
      if (compared[c] == idx) return k + static_cast<int>(c);
    return -1;
  }
};

// expect, have_dst, have_chk: k + m flags (nonzero = expected / wanted / compared). On an error
// `t` is unspecified.
inline FeedError build_feed_tables(int k, int m, size_t S, const uint8_t* expect, const uint8_t* have_dst,
                                   const uint8_t* have_chk, FeedTables& t) {
  t = FeedTables();
  t.k = k;
  t.m = m;
  const int n = k + m;
  int ne = 0;
  for (int i = 0; i < n; ++i) ne += expect[i] != 0;
  if (ne < k) return FeedError::kTooFewShards;
  if (ne > k) return FeedError::kArg;
  for (int i = 0; i < n; ++i)
    if (expect[i] ? (have_dst[i] || have_chk[i]) : (have_dst[i] && have_chk[i])) return FeedError::kArg;
  std::vector<uint8_t> present(static_cast<size_t>(n)), row(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    present[static_cast<size_t>(i)] = expect[i] != 0;
    row[static_cast<size_t>(i)] = have_dst[i] || have_chk[i];
    if (have_chk[i]) t.compared.push_back(i);
    if (have_dst[i]) t.wanted.push_back(i);
  }
  t.rows = t.compared;
  t.rows.insert(t.rows.end(), t.wanted.begin(), t.wanted.end());
  if (t.R() > kFeedMaxRows) return FeedError::kUnsupported;
  if (S == 0) return FeedError::kNoData;
  // present = the expected set: valid = V, nothing to compare, and one row per index of `row`
  DecodePlan dp;
  if (!decode_plan(k, m, present.data(), row.data(), dp)) return FeedError::kSingular;
  t.inversions = 1;
  t.expect = dp.valid;
  const int R = t.R();
  t.C = Mat(R, k);
  for (int r = 0; r < R; ++r)
    for (size_t at = 0; at < dp.missing.size(); ++at)
      if (dp.missing[at] == t.rows[static_cast<size_t>(r)])
        std::memcpy(&t.C.at(r, 0), dp.rows.row(static_cast<int>(at)), static_cast<size_t>(k));
  t.arena.assign(static_cast<size_t>(t.positions()) * t.block_words(), 0);
  for (int p = 0; p < t.positions(); ++p)
    for (int r = 0; r < R; ++r) {
      const uint8_t c = p < k ? t.C.at(r, p) : static_cast<uint8_t>(r == p - k ? 1 : 0);
      perm_tables(c, &t.arena[static_cast<size_t>(p) * t.block_words() + static_cast<size_t>(r) * kTabWords]);
    }
  return FeedError::kOk;
}

}  // namespace callfs
