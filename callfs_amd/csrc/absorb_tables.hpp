// Host-side tables of an absorb object (rs_absorb_create): the m parity rows of
// one object of k data shards of S bytes, into which ranges of the object's body are folded as
// they arrive. With P = rows k..n-1 of the encoding matrix (gf256.hpp encode_matrix), the arena
// holds per data shard i one block of m x 5 words, the v_perm tables (perm_tables) of P[.][i]:
// [k][m][kTabWords]. A launch over the body range [off, off + len) is an overwrite of that range
// whose old bytes are zero: overwrite_plan cuts the columns it touches into at most three
// intervals of consecutive shards, and absorb_plan adds what the kernel needs to find a block's
// interval, the running block counts at kAbsorbTileBytes columns per block. Plain C++ with no HIP
// dependence: tests/native/absorb_tables_test.cpp builds it with g++ on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "gf256.hpp"
#include "overwrite_plan.hpp"

namespace callfs {

constexpr int kAbsorbMaxRows = 16;
constexpr int kAbsorbMaxIntervals = 3;
// columns of one interval that one block of an absorb launch covers (= kFeedTileBytes)
constexpr uint32_t kAbsorbTileBytes = 4096;

// What build_absorb_tables refuses, in the order it checks: more than kAbsorbMaxRows parity rows
// (kUnsupported), then a zero size (kNoData); kSingular cannot happen for k + m <= 256.
enum class AbsorbError { kOk, kUnsupported, kNoData, kSingular };

struct AbsorbTables {
  int k = 0, m = 0;
  Mat P;                        // m x k: parity row j's coefficient of data shard i
  std::vector<uint32_t> arena;  // [k][m][kTabWords]
  size_t block_words() const { return static_cast<size_t>(m) * kTabWords; }
};

// The profile (k, m >= 1, k + m <= 256) is the caller's to check. On an error `t` is unspecified.
inline AbsorbError build_absorb_tables(int k, int m, size_t S, AbsorbTables& t) {
  t = AbsorbTables();
  t.k = k;
  t.m = m;
  if (m > kAbsorbMaxRows) return AbsorbError::kUnsupported;
  if (S == 0) return AbsorbError::kNoData;
  Mat E;
  if (!encode_matrix(k, m, E)) return AbsorbError::kSingular;
  t.P = Mat(m, k);
  for (int j = 0; j < m; ++j) std::memcpy(&t.P.at(j, 0), E.row(k + j), static_cast<size_t>(k));
  t.arena.assign(static_cast<size_t>(k) * t.block_words(), 0);
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < m; ++j)
      perm_tables(t.P.at(j, i), &t.arena[static_cast<size_t>(i) * t.block_words() + static_cast<size_t>(j) * kTabWords]);
  return AbsorbError::kOk;
}

// One launch: the intervals of overwrite_plan and, per interval, the number of blocks up to and
// including its own (end[q]; an unused interval repeats its predecessor's). Block b belongs to
// interval (b >= end[0]) + (b >= end[1]); grid = end[2].
struct AbsorbInterval {
  uint64_t col0 = 0, col1 = 0;  // columns [col0, col1)
  int32_t shard0 = 0, shard1 = 0;  // data shards shard0 .. shard1 inclusive
};

struct AbsorbPlan {
  AbsorbInterval iv[kAbsorbMaxIntervals];
  uint32_t end[kAbsorbMaxIntervals] = {0, 0, 0};
  int n = 0;
  uint32_t grid() const { return end[kAbsorbMaxIntervals - 1]; }
};

// False for what overwrite_plan refuses (an empty range, one outside [0, k * S)) and for a grid of
// 2^31 blocks or more. `scratch` is overwrite_plan's vector: a caller that keeps it allocates
// nothing per launch after the first.
inline bool absorb_plan(int k, size_t S, uint64_t off, uint64_t len, AbsorbPlan& p,
                        std::vector<OverwriteInterval>& scratch) {
  p = AbsorbPlan();
  if (!overwrite_plan(k, S, off, len, scratch)) return false;
  if (scratch.size() > static_cast<size_t>(kAbsorbMaxIntervals)) return false;
  uint64_t blocks = 0;
  for (const OverwriteInterval& o : scratch) {
    AbsorbInterval& v = p.iv[p.n];
    v.col0 = o.col0;
    v.col1 = o.col1;
    v.shard0 = o.shard0;
    v.shard1 = o.shard1;
    blocks += (static_cast<uint64_t>(o.col1 - o.col0) + kAbsorbTileBytes - 1) / kAbsorbTileBytes;
    if (blocks > 0x7fffffffull) return false;
    p.end[p.n++] = static_cast<uint32_t>(blocks);
  }
  for (int q = p.n; q < kAbsorbMaxIntervals; ++q) p.end[q] = static_cast<uint32_t>(blocks);
  return true;
}

inline bool absorb_plan(int k, size_t S, uint64_t off, uint64_t len, AbsorbPlan& p) {
  std::vector<OverwriteInterval> scratch;
  return absorb_plan(k, S, off, len, p, scratch);
}

}  // namespace callfs
