// Host-side tables of a decode-check device plan (rs_plan_create_decode_check):
// a decode-idx plan (decode_idx_tables.hpp) whose stripes also name compared shards. A compared
// shard j has a check row, the syndrome accumulator
//   check[j] (^)= sum over the delivered expected v of C[j][v] * input[v]  ^  input[j] if delivered
// with C = E[.] * inv(E[V]) as for the wanted rows: a decode-idx row with one more unit
// coefficient, for shard j's own delivery. A pattern is (expected, wanted, compared, delivered);
// patterns are deduplicated in order of first appearance over the stripes in the launch. Pattern
// p's row list is wanted and compared, ascending, nrows[p] of them; its source list is delivered,
// ascending, nsrc[p] of them, expected and compared sources alike. An expected source's column is
// C[row][v]; a compared source j's column is the unit column, 1 in row j and 0 elsewhere. Per
// launch group of up to 16 rows the arena holds the columns' nibble tables, and cmask[p] has bit
// r set when row r of the group is a check row. A stripe is in the launch when it has a
// delivered shard and a row; a final plan's stripe also when it has a check row and nothing
// delivered (nsrc[p] == 0: the kernel only scans the accumulators). The k x k inversion is done
// once per expected set. Plain C++ with no HIP dependence:
// tests/native/decode_check_host_test.cpp builds it with g++ on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "decode_idx_tables.hpp"

namespace callfs {

// One launch group: DecodeIdxGroup over the patterns' row lists, and which rows are check rows.
struct DecodeCheckGroup : DecodeIdxGroup {
  std::vector<uint32_t> cmask;  // [P] bit r: row row0 + r of pattern p is a check row
};

struct DecodeCheckPattern {
  std::vector<int> expect;     // k indices, ascending (V)
  std::vector<int> rows;       // wanted and compared, ascending
  std::vector<uint8_t> check;  // [rows] 1 = a check row
  std::vector<int> delivered;  // ascending, expected and compared sources
  std::vector<int> col;        // position of each delivered shard in V, -1 for a compared one
  Mat C;                       // rows x delivered
};

struct DecodeCheckTables {
  int k = 0, m = 0, batch = 0;
  int cmax = 0;  // the largest delivered set (0: nothing delivered anywhere)
  int rmax = 0;  // the largest row list
  int inversions = 0;
  std::vector<DecodeCheckPattern> patterns;
  std::vector<uint32_t> nsrc;   // [P]
  std::vector<uint32_t> nrows;  // [P] over all groups
  std::vector<uint32_t> pat;    // [batch] (0 and never read where the stripe is in no launch)
  std::vector<uint8_t> has;     // [batch] stripe b is in the launch
  std::vector<uint64_t> size;   // [batch]
  std::vector<DecodeCheckGroup> groups;
  TileMap map;
  // What a launch moves, summed over the stripes in it: size * (delivered + 2 wanted) in merge
  // mode and size * (delivered + wanted) in store mode, plus per check row twice its size in a
  // non-final merge, once in a non-final store or a final merge, nothing in a final store.
  // Indexed by (final ? 2 : 0) + (store ? 1 : 0).
  uint64_t bytes[4] = {0, 0, 0, 0};
  int P() const { return static_cast<int>(patterns.size()); }
};

// expect, have_in, have_dst, have_chk: batch * (k + m) flags (nonzero = expected / delivered with
// this plan / wanted / compared). Refuses what build_decode_idx_tables refuses, in its order; the
// misplaced pointers are an input at an index that is neither expected nor compared, a dst or a
// check at an expected index, and a check and a dst at one index (kArg); a zero size on a stripe
// in the launch is kNoData. On an error `t` is unspecified.
inline DecodeIdxError build_decode_check_tables(int k, int m, int batch, const size_t* sizes,
                                                const uint8_t* expect, const uint8_t* have_in,
                                                const uint8_t* have_dst, const uint8_t* have_chk,
                                                bool final, DecodeCheckTables& t) {
  t = DecodeCheckTables();
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
      if (expect[at] ? (have_dst[at] || have_chk[at]) : ((have_in[at] && !have_chk[at]) || (have_chk[at] && have_dst[at])))
        return DecodeIdxError::kArg;
    }
  t.pat.assign(B, 0);
  t.has.assign(B, 0);
  t.size.assign(B, 0);
  std::vector<size_t> mapped(B, 1);  // a skipped stripe's size is never read
  for (size_t b = 0; b < B; ++b) {
    bool in = false, row = false, chk = false;
    for (int i = 0; i < n; ++i) {
      in |= have_in[b * n + i] != 0;
      row |= have_dst[b * n + i] != 0 || have_chk[b * n + i] != 0;
      chk |= have_chk[b * n + i] != 0;
    }
    t.size[b] = sizes[b];
    if (!((in && row) || (final && chk))) continue;
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
    DecodeCheckPattern p;
    for (int i = 0; i < n; ++i) {
      const size_t at = b * n + i;
      if (expect[at]) {
        ekey[static_cast<size_t>(i)] = '1';
        if (have_in[at]) {
          p.delivered.push_back(i);
          p.col.push_back(static_cast<int>(p.expect.size()));
        }
        p.expect.push_back(i);
      } else {
        if (have_in[at]) {
          p.delivered.push_back(i);
          p.col.push_back(-1);
        }
        if (have_dst[at] || have_chk[at]) {
          p.rows.push_back(i);
          p.check.push_back(have_chk[at] != 0);
        }
      }
      key[static_cast<size_t>(i)] = static_cast<char>('0' + (expect[at] ? 1 : 0) + (have_in[at] ? 2 : 0) +
                                                      (have_dst[at] ? 4 : 0) + (have_chk[at] ? 8 : 0));
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
      p.C = Mat(static_cast<int>(p.rows.size()), static_cast<int>(p.delivered.size()));
      for (size_t r = 0; r < p.rows.size(); ++r) {
        Mat er(1, k);
        std::memcpy(&er.at(0, 0), E.row(p.rows[r]), k);
        const Mat row = matmul(er, D);
        for (size_t c = 0; c < p.delivered.size(); ++c)
          p.C.at(static_cast<int>(r), static_cast<int>(c)) =
              p.col[c] >= 0 ? row.at(0, p.col[c])
                            : static_cast<uint8_t>(p.delivered[c] == p.rows[r] && p.check[r] ? 1 : 0);
      }
      it = seen.emplace(key, static_cast<uint32_t>(t.patterns.size())).first;
      t.cmax = std::max(t.cmax, static_cast<int>(p.delivered.size()));
      t.rmax = std::max(t.rmax, static_cast<int>(p.rows.size()));
      t.nsrc.push_back(static_cast<uint32_t>(p.delivered.size()));
      t.nrows.push_back(static_cast<uint32_t>(p.rows.size()));
      t.patterns.push_back(std::move(p));
    }
    t.pat[b] = it->second;
    const DecodeCheckPattern& pt = t.patterns[it->second];
    const uint64_t c = pt.delivered.size();
    const uint64_t nc = static_cast<uint64_t>(std::count(pt.check.begin(), pt.check.end(), 1));
    const uint64_t w = pt.rows.size() - nc;
    uint64_t most;
    if (__builtin_mul_overflow(static_cast<uint64_t>(sizes[b]), c + 2 * (w + nc), &most) ||
        __builtin_add_overflow(t.bytes[0], most, &t.bytes[0]))
      return DecodeIdxError::kTooManyTiles;
    t.bytes[1] += static_cast<uint64_t>(sizes[b]) * (c + w + nc);
    t.bytes[2] += static_cast<uint64_t>(sizes[b]) * (c + 2 * w + nc);
    t.bytes[3] += static_cast<uint64_t>(sizes[b]) * (c + w);
  }
  switch (build_tile_map(batch, mapped.data(), t.has.data(), t.map)) {
    case TableError::kOk: break;
    case TableError::kNoData: return DecodeIdxError::kNoData;
    case TableError::kSingular: return DecodeIdxError::kSingular;
    default: return DecodeIdxError::kTooManyTiles;
  }
  const size_t P = t.patterns.size();
  for (int g0 = 0; g0 < t.rmax; g0 += kMixedRowsPerLaunch) {
    DecodeCheckGroup g;
    g.row0 = g0;
    g.R = std::min(kMixedRowsPerLaunch, t.rmax - g0);
    const size_t per_shard = 32u * static_cast<size_t>(nibble_width(g.R));
    g.tab_stride = (static_cast<size_t>(t.cmax) * per_shard + 255) / 256 * 256;
    g.arena.assign(P * g.tab_stride, 0);
    g.nrows.assign(P, 0);
    g.cmask.assign(P, 0);
    for (size_t p = 0; p < P; ++p) {
      const DecodeCheckPattern& pt = t.patterns[p];
      const int have = std::max(0, std::min(g.R, static_cast<int>(pt.rows.size()) - g0));
      g.nrows[p] = static_cast<uint32_t>(have);
      for (int r = 0; r < have; ++r)
        if (pt.check[static_cast<size_t>(g0 + r)]) g.cmask[p] |= 1u << r;
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
