// Host-side tables of a decode-repair device plan (rs_plan_create_decode_repair, DESIGN.md
// §5.16): a final decode-check plan (decode_check_tables.hpp) whose last launch also names the
// corrupt shard of a mismatching byte column from the finished check rows, repairs the wanted
// rows within the launch and hands the error values back through `fix` buffers. The
// patterns are build_decode_check_tables' with one change: pattern p's row list is its compared
// indices ascending, then its wanted indices ascending, so that the r' syndromes of a column are
// bytes 0..r'-1 of the packed accumulator -- what locate_correct (locate_tables.hpp) reads with
// static positions -- and cmask[p] is the low r' bits. A stripe has at most 16 rows, r' + w <=
// 16: every syndrome and every wanted row of a column meet in one block, and there is one launch
// group. Beside the nibble tables each pattern holds a locate block in locate_tables.hpp's
// layout (kLocRatio, kLocMap, kLocG, stride locate_stride(k)) over G = E[rows] . inv(E[V]), all k
// expected positions whether delivered with this plan or not: the ratio table from check rows 0
// and 1, the position map V then the compared shards, and G by column over all rows of the group
// (check rows first, then wanted), so that column j's 16 bytes serve the confirmation and the
// repair of the wanted rows alike. The log / exp block is the locate plans' (kLocGfBytes). The
// fix pointers go into a per-stripe table of k + 16 entries indexed by position (fix_slot).
// Plain C++ with no HIP dependence: tests/native/decode_repair_host_test.cpp builds it with g++.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "decode_check_tables.hpp"
#include "locate_tables.hpp"

namespace callfs {

// What build_decode_repair_tables refuses, in the order it checks: over the whole batch the
// expected counts (fewer than k: kTooFewShards, more: kArg), then the misplaced pointers
// (build_decode_check_tables' and a fix at an index that is neither expected nor compared: kArg),
// then a stripe with more than 16 rows (kUnsupported), then a zero size on a stripe in the launch
// (kNoData); kTooManyTiles and kSingular as for the other tables.
enum class DecodeRepairError { kOk, kArg, kTooFewShards, kUnsupported, kNoData, kTooManyTiles, kSingular };

constexpr int kRepairRows = kLocateRows;  // rows per stripe, compared and wanted together
// pointers per stripe in the fix table: position j < k is expected shard V[j], k + x compared shard x
CALLFS_HD inline size_t fix_slots(int k) { return static_cast<size_t>(k) + kRepairRows; }

struct DecodeRepairTables {
  // patterns (rows: compared then wanted), pat, sizes, the tile map, bytes and at most one launch
  // group, laid out as finish_decode_plan and the final decode-check launch read them
  DecodeCheckTables c;
  std::vector<uint32_t> nchk;  // [P] r' of pattern p: rows [0, r') are its check rows
  std::vector<uint8_t> gf;     // kLocGfBytes, shared by every pattern
  size_t stride = 0;           // locate_stride(k)
  std::vector<uint8_t> loc;    // [P][stride]
};

// expect, have_in, have_dst, have_chk, have_fix: batch * (k + m) flags. On an error `t` is
// unspecified.
inline DecodeRepairError build_decode_repair_tables(int k, int m, int batch, const size_t* sizes,
                                                    const uint8_t* expect, const uint8_t* have_in,
                                                    const uint8_t* have_dst, const uint8_t* have_chk,
                                                    const uint8_t* have_fix, DecodeRepairTables& t) {
  t = DecodeRepairTables();
  const int n = k + m;
  const size_t B = static_cast<size_t>(batch);
  for (size_t b = 0; b < B; ++b) {
    int ne = 0;
    for (int i = 0; i < n; ++i) ne += expect[b * n + i] != 0;
    if (ne < k) return DecodeRepairError::kTooFewShards;
    if (ne > k) return DecodeRepairError::kArg;
  }
  for (size_t b = 0; b < B; ++b)
    for (int i = 0; i < n; ++i) {
      const size_t at = b * n + i;
      if (expect[at] ? (have_dst[at] || have_chk[at])
                     : ((have_in[at] && !have_chk[at]) || (have_chk[at] && have_dst[at]) ||
                        (have_fix[at] && !have_chk[at])))
        return DecodeRepairError::kArg;
    }
  for (size_t b = 0; b < B; ++b) {
    int rows = 0;
    for (int i = 0; i < n; ++i) rows += have_dst[b * n + i] != 0 || have_chk[b * n + i] != 0;
    if (rows > kRepairRows) return DecodeRepairError::kUnsupported;
  }
  switch (build_decode_check_tables(k, m, batch, sizes, expect, have_in, have_dst, have_chk, /*final=*/true, t.c)) {
    case DecodeIdxError::kOk: break;
    case DecodeIdxError::kArg: return DecodeRepairError::kArg;
    case DecodeIdxError::kTooFewShards: return DecodeRepairError::kTooFewShards;
    case DecodeIdxError::kNoData: return DecodeRepairError::kNoData;
    case DecodeIdxError::kTooManyTiles: return DecodeRepairError::kTooManyTiles;
    case DecodeIdxError::kSingular: return DecodeRepairError::kSingular;
  }
  const GF& g = gf();
  t.gf.assign(kLocGfBytes, 0);
  for (size_t i = 0; i < 256; ++i) t.gf[i] = g.log[i];
  for (size_t i = 0; i < 512; ++i) t.gf[256 + i] = g.exp[i];
  t.stride = locate_stride(k);
  const size_t P = t.c.patterns.size();
  t.nchk.assign(P, 0);
  t.loc.assign(P * t.stride, 0);
  if (P == 0) return DecodeRepairError::kOk;
  // every pattern has 1..16 rows: one launch group
  DecodeCheckGroup& grp = t.c.groups[0];
  const size_t per_shard = 32u * static_cast<size_t>(nibble_width(grp.R));
  Mat E;
  if (!encode_matrix(k, m, E)) return DecodeRepairError::kSingular;
  std::map<std::vector<int>, Mat> inverse;  // per expected set: inv(E[V])
  for (size_t p = 0; p < P; ++p) {
    DecodeCheckPattern& pt = t.c.patterns[p];
    const int R = static_cast<int>(pt.rows.size());
    // compared rows first: a stable partition keeps both halves ascending
    std::vector<int> perm(static_cast<size_t>(R));
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_partition(perm.begin(), perm.end(), [&](int r) { return pt.check[static_cast<size_t>(r)] != 0; });
    DecodeCheckPattern q = pt;
    for (int r = 0; r < R; ++r) {
      const int from = perm[static_cast<size_t>(r)];
      q.rows[static_cast<size_t>(r)] = pt.rows[static_cast<size_t>(from)];
      q.check[static_cast<size_t>(r)] = pt.check[static_cast<size_t>(from)];
      for (int c = 0; c < pt.C.cols; ++c) q.C.at(r, c) = pt.C.at(from, c);
    }
    pt = std::move(q);
    const int rc = static_cast<int>(std::count(pt.check.begin(), pt.check.end(), 1));
    t.nchk[p] = static_cast<uint32_t>(rc);
    grp.cmask[p] = rc ? (1u << rc) - 1u : 0u;
    for (size_t c = 0; c < pt.delivered.size(); ++c) {
      uint8_t col[kMixedRowsPerLaunch] = {0};
      for (int r = 0; r < R; ++r) col[r] = pt.C.at(r, static_cast<int>(c));
      nibble_tables(col, grp.R, &grp.arena[p * grp.tab_stride + c * per_shard]);
    }
    // the locate block: G over all k expected positions and all rows of the pattern
    auto inv = inverse.find(pt.expect);
    if (inv == inverse.end()) {
      Mat sub(k, k), D;
      for (int r = 0; r < k; ++r) std::memcpy(&sub.at(r, 0), E.row(pt.expect[static_cast<size_t>(r)]), k);
      if (!invert(sub, D)) return DecodeRepairError::kSingular;
      inv = inverse.emplace(pt.expect, std::move(D)).first;
    }
    uint8_t* blk = &t.loc[p * t.stride];
    for (size_t r = 0; r < 256; ++r) blk[kLocRatio + r] = 0xff;
    for (int j = 0; j < k; ++j) blk[kLocMap + static_cast<size_t>(j)] = static_cast<uint8_t>(pt.expect[static_cast<size_t>(j)]);
    for (int x = 0; x < rc; ++x)
      blk[kLocMap + static_cast<size_t>(k + x)] = static_cast<uint8_t>(pt.rows[static_cast<size_t>(x)]);
    for (int r = 0; r < R; ++r) {
      Mat er(1, k);
      std::memcpy(&er.at(0, 0), E.row(pt.rows[static_cast<size_t>(r)]), k);
      const Mat row = matmul(er, inv->second);
      for (int j = 0; j < k; ++j) blk[kLocG + static_cast<size_t>(j) * kLocateRows + static_cast<size_t>(r)] = row.at(0, j);
    }
    if (rc < 2) continue;
    for (int j = 0; j < k; ++j) {
      const uint8_t* gj = blk + kLocG + static_cast<size_t>(j) * kLocateRows;
      blk[kLocRatio + g.mul[gj[1]][g.inv(gj[0])]] = static_cast<uint8_t>(j);
    }
  }
  return DecodeRepairError::kOk;
}

// g times each of the four bytes of w in GF(2^8) mod 0x11D, by Horner's rule over the bits of g
// on the four bytes at once: equal to locate_mul byte by byte, with no table read. (The vector
// path repairs 16 bytes of a wanted row with four of these, g changing from row to row. Sixteen
// chains of table loads in flight took 40 registers more than the clean path holds, and so did
// the form that doubles w bit by bit, whose eight multiples of w do not depend on the row and
// were kept across the row loop.)
CALLFS_HD inline uint32_t repair_mul_word(uint32_t g, uint32_t w) {
  uint32_t o = 0;
  CALLFS_UNROLL
  for (int bit = 7; bit >= 0; --bit) {
    o = ((o & 0x7f7f7f7fu) << 1) ^ (((o >> 7) & 0x01010101u) * 0x1du);
    o ^= (g >> bit) & 1u ? w : 0u;
  }
  return o;
}

// One byte column by the rule, as the kernel and the CPU tests run it. s: the
// rows' final values packed one per byte, check rows in bytes [0, nchk), wanted rows in
// [nchk, rows); pt: the pattern's locate block. Returns locate_correct's verdict over the check
// rows; with a shard verdict `pos` is the shard's position (fix_slots' index) and `value` its
// error, and for an expected shard the wanted bytes of s have the error's share G[r][pos] . value
// taken out.
template <int NW>
CALLFS_HD inline uint32_t repair_column(uint32_t (&s)[NW], int nchk, int rows, int k, const uint8_t* gf,
                                        const uint8_t* pt, uint32_t& pos, uint32_t& value) {
  const uint32_t v = locate_correct(s, nchk, k, gf, pt, pos, value);
  if (v < 256u && pos < static_cast<uint32_t>(k)) {
    // one copy of the multiply, in a loop over the wanted rows that stays a loop, with the
    // row's word picked by selects: in the kernel the syndromes stay in registers and the slow
    // path holds a handful more
    const uint8_t* gj = pt + kLocG + static_cast<size_t>(pos) * kLocateRows;
    CALLFS_NO_UNROLL
    for (int r = nchk; r < rows; ++r) {
      const uint32_t add = locate_mul(gf, gj[r], value) << (8 * (r & 3));
      CALLFS_UNROLL
      for (int w = 0; w < NW; ++w)
        if ((r >> 2) == w) s[w] ^= add;
    }
  }
  return v;
}

}  // namespace callfs
