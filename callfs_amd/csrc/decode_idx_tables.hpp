// Host-side tables of a decode-idx device plan (rs_plan_create_decode_idx):
// upstream DecodeIdx over a batch in which every stripe has its own shard size, its own k
// expected shards, its own wanted shards and its own shards delivered with this plan. A pattern
// is the triple (expected set, wanted set, delivered set); patterns are deduplicated in order of
// first appearance over the stripes that have both a delivered and a wanted shard. With V the
// expected indices in ascending order and C = E[w] . inv(E[V]) (the row rs_decode_rows returns
// for a presence mask equal to the expected set), pattern p has nsrc[p] delivered shards
// (ascending), nrows[p] wanted shards (ascending), and per launch group of up to 16 wanted rows
// the nibble tables of C[w][v] for the delivered columns alone. One arena per launch group holds
// the patterns' tables at a pitch sized for the largest delivered set; group g holds rows
// [16 g, 16 g + 16) of every pattern's wanted list, g.nrows[p] of them (0 when the pattern has
// no row that far). The k x k inversion is done once per expected set. The tile map
// (ragged_tables.hpp) covers the stripes with both a delivered and a wanted shard; any other
// stripe has no tile, and a batch with none launches nothing. Plain C++ with no HIP dependence:
// tests/native/decode_idx_host_test.cpp builds it with g++ on the CPU.
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

// What build_decode_idx_tables refuses, in the order it checks: over the whole batch the expected
// counts first (fewer than k: kTooFewShards, more: kArg), then the misplaced pointers (an input
// at an index that is not expected, a dst at one that is: kArg), then a zero size on a stripe
// with both an input and a dst (kNoData); kTooManyTiles and kSingular as for the other tables.
enum class DecodeIdxError { kOk, kArg, kTooFewShards, kNoData, kTooManyTiles, kSingular };

// One launch group: rows [row0, row0 + nrows[p]) of every pattern's wanted list.
struct DecodeIdxGroup {
  int row0 = 0;
  int R = 0;                    // the most rows a pattern has in this group, 1..16
  size_t tab_stride = 0;        // cmax * 32 * nibble_width(R), rounded up to 256
  std::vector<uint32_t> nrows;  // [P] rows of pattern p in this group, 0..R
  std::vector<uint8_t> arena;   // [P][cmax][32][W]: pattern p's tables at p * tab_stride
};

struct DecodeIdxPattern {
  std::vector<int> expect;     // k indices, ascending (V)
  std::vector<int> wanted;     // ascending
  std::vector<int> delivered;  // ascending
  std::vector<int> col;        // position of each delivered shard in V
  Mat C;                       // wanted x delivered
};

struct DecodeIdxTables {
  int k = 0, m = 0, batch = 0;
  int cmax = 0;  // the largest delivered set (0: no stripe in a launch)
  int rmax = 0;  // the largest wanted set
  int inversions = 0;  // distinct expected sets inverted
  std::vector<DecodeIdxPattern> patterns;
  std::vector<uint32_t> nsrc;   // [P]
  std::vector<uint32_t> nrows;  // [P] over all groups
  std::vector<uint32_t> pat;    // [batch] (0 and never read where the stripe is in no launch)
  std::vector<uint8_t> has;     // [batch] stripe b has both a delivered and a wanted shard
  std::vector<uint64_t> size;   // [batch]
  std::vector<DecodeIdxGroup> groups;
  TileMap map;
  // sum over the stripes in the launch of size * (c_b + 2 r_b) and size * (c_b + r_b)
  uint64_t bytes_merge = 0, bytes_store = 0;
  int P() const { return static_cast<int>(patterns.size()); }
};

// expect, have_in, have_dst: batch * (k + m) flags (nonzero = expected / delivered with this
// plan / wanted). On an error `t` is unspecified.
inline DecodeIdxError build_decode_idx_tables(int k, int m, int batch, const size_t* sizes,
                                              const uint8_t* expect, const uint8_t* have_in,
                                              const uint8_t* have_dst, DecodeIdxTables& t) {
  t = DecodeIdxTables();
  t.k = k;
  t.m = m;
  t.batch = batch;
  const int n = k + m;
  const size_t B = static_cast<size_t>(batch);
  for (size_t b = 0; b < B; ++b) {
    int ne = 0;
    for (int i = 0; i < n; ++i) ne += expect[b * n + i] != 0;
    if (ne < k) return DecodeIdxError::kTooFewShards;
    if (ne > k) return DecodeIdxError::kArg;
  }
  for (size_t b = 0; b < B; ++b)
    for (int i = 0; i < n; ++i) {
      const size_t at = b * n + i;
      if (expect[at] ? have_dst[at] != 0 : have_in[at] != 0) return DecodeIdxError::kArg;
    }
  t.pat.assign(B, 0);
  t.has.assign(B, 0);
  t.size.assign(B, 0);
  std::vector<size_t> mapped(B, 1);  // a skipped stripe's size is never read
  for (size_t b = 0; b < B; ++b) {
    bool in = false, out = false;
    for (int i = 0; i < n; ++i) {
      in |= have_in[b * n + i] != 0;
      out |= have_dst[b * n + i] != 0;
    }
    t.size[b] = sizes[b];
    if (!in || !out) continue;
    if (sizes[b] == 0) return DecodeIdxError::kNoData;
    t.has[b] = 1;
    mapped[b] = sizes[b];
  }
  Mat E;
  std::map<std::string, uint32_t> seen;
  std::map<std::string, Mat> inverse;  // per expected set: inv(E[V])
  for (size_t b = 0; b < B; ++b) {
    if (!t.has[b]) continue;
    std::string ekey(static_cast<size_t>(n), '0'), key(static_cast<size_t>(n), '0');
    DecodeIdxPattern p;
    for (int i = 0; i < n; ++i) {
      const size_t at = b * n + i;
      if (expect[at]) {
        ekey[static_cast<size_t>(i)] = '1';
        if (have_in[at]) {
          p.delivered.push_back(i);
          p.col.push_back(static_cast<int>(p.expect.size()));
        }
        p.expect.push_back(i);
      } else if (have_dst[at]) {
        p.wanted.push_back(i);
      }
      key[static_cast<size_t>(i)] = static_cast<char>('0' + (expect[at] ? 1 : 0) + (have_in[at] ? 2 : 0) +
                                                      (have_dst[at] ? 4 : 0));
    }
    auto it = seen.find(key);
    if (it == seen.end()) {
      if (E.rows == 0 && !encode_matrix(k, m, E)) return DecodeIdxError::kSingular;
      auto inv = inverse.find(ekey);
      if (inv == inverse.end()) {
        Mat sub(k, k), D;
        for (int r = 0; r < k; ++r) std::memcpy(&sub.at(r, 0), E.row(p.expect[static_cast<size_t>(r)]), k);
        if (!invert(sub, D)) return DecodeIdxError::kSingular;
        inv = inverse.emplace(ekey, std::move(D)).first;
        ++t.inversions;
      }
      const Mat& D = inv->second;
      p.C = Mat(static_cast<int>(p.wanted.size()), static_cast<int>(p.delivered.size()));
      for (size_t r = 0; r < p.wanted.size(); ++r) {
        Mat er(1, k);
        std::memcpy(&er.at(0, 0), E.row(p.wanted[r]), k);
        const Mat row = matmul(er, D);  // a data index: E's row is a unit row, so this is D's row
        for (size_t c = 0; c < p.delivered.size(); ++c)
          p.C.at(static_cast<int>(r), static_cast<int>(c)) = row.at(0, p.col[c]);
      }
      it = seen.emplace(key, static_cast<uint32_t>(t.patterns.size())).first;
      t.cmax = std::max(t.cmax, static_cast<int>(p.delivered.size()));
      t.rmax = std::max(t.rmax, static_cast<int>(p.wanted.size()));
      t.nsrc.push_back(static_cast<uint32_t>(p.delivered.size()));
      t.nrows.push_back(static_cast<uint32_t>(p.wanted.size()));
      t.patterns.push_back(std::move(p));
    }
    t.pat[b] = it->second;
    const uint64_t c = t.nsrc[it->second], r = t.nrows[it->second];
    uint64_t add;
    if (__builtin_mul_overflow(static_cast<uint64_t>(sizes[b]), c + 2 * r, &add) ||
        __builtin_add_overflow(t.bytes_merge, add, &t.bytes_merge))
      return DecodeIdxError::kTooManyTiles;
    t.bytes_store += static_cast<uint64_t>(sizes[b]) * (c + r);
  }
  switch (build_tile_map(batch, mapped.data(), t.has.data(), t.map)) {
    case TableError::kOk: break;
    case TableError::kNoData: return DecodeIdxError::kNoData;
    case TableError::kSingular: return DecodeIdxError::kSingular;
    default: return DecodeIdxError::kTooManyTiles;
  }
  const size_t P = t.patterns.size();
  for (int g0 = 0; g0 < t.rmax; g0 += kMixedRowsPerLaunch) {
    DecodeIdxGroup g;
    g.row0 = g0;
    g.R = std::min(kMixedRowsPerLaunch, t.rmax - g0);
    const size_t per_shard = 32u * static_cast<size_t>(nibble_width(g.R));
    g.tab_stride = (static_cast<size_t>(t.cmax) * per_shard + 255) / 256 * 256;
    g.arena.assign(P * g.tab_stride, 0);
    g.nrows.assign(P, 0);
    for (size_t p = 0; p < P; ++p) {
      const DecodeIdxPattern& pt = t.patterns[p];
      const int have = std::max(0, std::min(g.R, static_cast<int>(pt.wanted.size()) - g0));
      g.nrows[p] = static_cast<uint32_t>(have);
      if (have == 0) continue;
      for (size_t c = 0; c < pt.delivered.size(); ++c) {
        uint8_t col[kMixedRowsPerLaunch] = {0};
        for (int r = 0; r < have; ++r) col[r] = pt.C.at(g0 + r, static_cast<int>(c));
        nibble_tables(col, g.R, &g.arena[p * g.tab_stride + c * per_shard]);
      }
    }
    t.groups.push_back(std::move(g));
  }
  return DecodeIdxError::kOk;
}

}  // namespace callfs
