// Host-side tables of an update device plan (rs_plan_create_update): upstream
// Update / EncodeIdx over a batch in which every stripe has its own shard size and its own set
// of changed data shards. The changed sets are deduplicated into patterns in order of first
// appearance; pattern p has nsrc[p] changed shards (ascending) and, per launch group of up to
// 16 parity rows, the nibble tables of P[j][i] for those shards alone, P the parity rows of the
// encode matrix. One arena per launch group holds the patterns' tables at a pitch sized for
// the largest changed set. The tile map (ragged_tables.hpp) covers the stripes with a changed
// shard; a stripe with none has no tile, and a batch with none launches nothing. Plain C++ with
// no HIP dependence: tests/native/update_host_test.cpp builds it with g++ on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "gf256.hpp"
#include "ragged_tables.hpp"

namespace callfs {

// One launch group: parity rows [row0, row0 + R).
struct UpdateGroup {
  int row0 = 0;
  int R = 0;
  size_t tab_stride = 0;       // cmax * 32 * nibble_width(R), rounded up to 256
  std::vector<uint8_t> arena;  // [P][cmax][32][W]: pattern p's tables at p * tab_stride
};

struct UpdateTables {
  int k = 0, m = 0, batch = 0;
  int cmax = 0;                            // the largest changed set (0: nothing changed)
  std::vector<std::vector<int>> patterns;  // P distinct non-empty changed sets, ascending indices
  std::vector<uint32_t> nsrc;              // [P] = patterns[p].size()
  std::vector<uint32_t> pat;               // [batch] stripe b's pattern (0 and never read where nothing changed)
  std::vector<uint8_t> has;                // [batch] stripe b has a changed shard
  std::vector<uint64_t> size;              // [batch]
  std::vector<UpdateGroup> groups;         // none when nothing changed
  TileMap map;                             // over the stripes with a changed shard
  // sum over those stripes of size * (c_b * (2: old and new | 1: EncodeIdx) + 2 m)
  uint64_t bytes_pair = 0, bytes_single = 0;
  int P() const { return static_cast<int>(patterns.size()); }
};

// changed: batch * k flags (nonzero = changed). kNoData: a stripe with a changed shard has
// size 0; kTooManyTiles: more tiles than a grid holds (or a byte count past 2^64);
// kSingular: no encode matrix (cannot happen for k + m <= 256). On an error `t` is unspecified.
inline TableError build_update_tables(int k, int m, int batch, const size_t* sizes,
                                      const uint8_t* changed, UpdateTables& t) {
  t = UpdateTables();
  t.k = k;
  t.m = m;
  t.batch = batch;
  t.pat.assign(static_cast<size_t>(batch), 0);
  t.has.assign(static_cast<size_t>(batch), 0);
  t.size.assign(static_cast<size_t>(batch), 0);
  std::map<std::string, uint32_t> seen;
  std::vector<size_t> mapped(static_cast<size_t>(batch), 1);  // a skipped stripe's size is never read
  for (int b = 0; b < batch; ++b) {
    const uint8_t* f = changed + static_cast<size_t>(b) * k;
    std::string key(static_cast<size_t>(k), '0');
    std::vector<int> idx;
    for (int i = 0; i < k; ++i)
      if (f[i]) {
        key[static_cast<size_t>(i)] = '1';
        idx.push_back(i);
      }
    t.size[static_cast<size_t>(b)] = sizes[b];
    if (idx.empty()) continue;
    if (sizes[b] == 0) return TableError::kNoData;
    t.has[static_cast<size_t>(b)] = 1;
    mapped[static_cast<size_t>(b)] = sizes[b];
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(key, static_cast<uint32_t>(t.patterns.size())).first;
      t.cmax = std::max(t.cmax, static_cast<int>(idx.size()));
      t.nsrc.push_back(static_cast<uint32_t>(idx.size()));
      t.patterns.push_back(idx);
    }
    t.pat[static_cast<size_t>(b)] = it->second;
    const uint64_t c = idx.size();
    uint64_t add;
    if (__builtin_mul_overflow(static_cast<uint64_t>(sizes[b]), 2 * c + 2 * static_cast<uint64_t>(m), &add) ||
        __builtin_add_overflow(t.bytes_pair, add, &t.bytes_pair))
      return TableError::kTooManyTiles;
    t.bytes_single += static_cast<uint64_t>(sizes[b]) * (c + 2 * static_cast<uint64_t>(m));
  }
  if (const TableError e = build_tile_map(batch, mapped.data(), t.has.data(), t.map); e != TableError::kOk)
    return e;
  if (t.patterns.empty()) return TableError::kOk;
  Mat E;
  if (!encode_matrix(k, m, E)) return TableError::kSingular;
  const size_t P = t.patterns.size();
  for (int g0 = 0; g0 < m; g0 += kMixedRowsPerLaunch) {
    UpdateGroup g;
    g.row0 = g0;
    g.R = std::min(kMixedRowsPerLaunch, m - g0);
    const size_t per_shard = 32u * static_cast<size_t>(nibble_width(g.R));
    g.tab_stride = (static_cast<size_t>(t.cmax) * per_shard + 255) / 256 * 256;
    g.arena.assign(P * g.tab_stride, 0);
    for (size_t p = 0; p < P; ++p)
      for (size_t c = 0; c < t.patterns[p].size(); ++c) {
        uint8_t col[kMixedRowsPerLaunch] = {0};
        for (int r = 0; r < g.R; ++r) col[r] = E.at(k + g0 + r, t.patterns[p][c]);
        nibble_tables(col, g.R, &g.arena[p * g.tab_stride + c * per_shard]);
      }
    t.groups.push_back(std::move(g));
  }
  return TableError::kOk;
}

}  // namespace callfs
