// Host-side tables of a locate plan (rs_plan_create_locate) and the rule
// that turns one byte column's parity syndromes into a verdict: which shard is corrupt there.
// A locate plan is a required plan (ragged_tables.hpp) in which nothing is written and every
// present shard beyond the first k is compared -- but for the 16 rows of one launch group:
// stripe b compares r'_b = min(present - k, 16) shards, later ones are neither read nor
// blamed, and a stripe with exactly k present shards has no row and is in no launch. Beside
// the nibble tables each pattern holds what the rule reads: its compare rows G = E[cmp] .
// inv(E[valid]) stored by column, the table from the ratio G[1][j] / G[0][j] to the position
// j, and the position -> shard index map over valid then cmp. E is MDS, so no entry of G is
// zero and for r' >= 2 the ratios are pairwise distinct.
// Plain C++ with no HIP dependence (tests/native/locate_host_test.cpp builds it with g++ on
// the CPU); locate_classify is the one function the kernel and the CPU test both run.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ragged_tables.hpp"

#if defined(__HIPCC__)
#define CALLFS_HD __host__ __device__
#else
#define CALLFS_HD
#endif
#if defined(__clang__)
#define CALLFS_UNROLL _Pragma("unroll")
#else
#define CALLFS_UNROLL _Pragma("GCC unroll 16")
#endif

namespace callfs {

constexpr int kLocateRows = kMixedRowsPerLaunch;  // compared shards examined per stripe
// verdicts of a column that are no shard index (shard indices are below 256)
constexpr uint32_t kLocateClean = 0xffffffffu;
constexpr uint32_t kLocateUnexplained = 0xfffffffeu;

// One pattern's block of the device tables, kLocStride(k) bytes:
constexpr size_t kLocRatio = 0;        // [256] ratio -> position in valid, 0xFF = none
constexpr size_t kLocMap = 256;        // [k + 16] position -> shard index: valid, then cmp
constexpr size_t kLocG = 256 + 272;    // [k][16] G by column: G[x][j] at j * 16 + x
inline size_t locate_stride(int k) { return kLocG + static_cast<size_t>(k) * kLocateRows; }
// The block every pattern shares: log[256], then exp[512] (exp[i] = 2^(i mod 255))
constexpr size_t kLocGfBytes = 768;

// Byte x of the packed syndromes (row x of the launch group in byte x & 3 of word x >> 2).
template <int NW>
CALLFS_HD inline uint32_t locate_byte(const uint32_t (&s)[NW], int x) {
  return (s[x >> 2] >> (8 * (x & 3))) & 0xffu;
}

// The verdict of one byte column. s: the `rows` syndromes s_x = stored_cmp[x] ^ (G[x] . valid),
// packed one per byte (bytes at and past `rows` are not read); gf: the shared log / exp block;
// pt: the pattern's block. Returns the shard index to blame, kLocateUnexplained or
// kLocateClean:
//   every s_x zero: clean. One row (rows < 2) cannot tell shards apart: unexplained. Exactly
//   one s_x nonzero: compared shard x. Every s_x nonzero: q = s_1 / s_0 names position j of
//   `valid` (or none: unexplained), e = s_0 / G[0][j], and shard valid[j] is blamed when
//   s_x = G[x][j] . e for every x >= 2. Anything else is unexplained.
// Over the k + rows examined shards a column with one corrupt byte is blamed on exactly that
// shard and a column with 2..rows-1 corrupt bytes on nobody (the code has distance rows + 1).
// Every loop is unrolled over the NW * 4 possible rows with static byte positions: in the
// kernel the syndromes stay in registers.
template <int NW>
CALLFS_HD inline uint32_t locate_classify(const uint32_t (&s)[NW], int rows, int k,
                                          const uint8_t* gf, const uint8_t* pt) {
  int nz = 0, first = 0;
  CALLFS_UNROLL
  for (int x = NW * 4 - 1; x >= 0; --x) {
    if (x < rows && locate_byte(s, x) != 0) {
      ++nz;
      first = x;
    }
  }
  if (nz == 0) return kLocateClean;
  if (rows < 2) return kLocateUnexplained;
  if (nz == 1) return pt[kLocMap + static_cast<size_t>(k) + first];
  if (nz != rows) return kLocateUnexplained;
  const uint8_t* lg = gf;
  const uint8_t* ex = gf + 256;
  const uint32_t s0 = locate_byte(s, 0), s1 = locate_byte(s, 1);
  const uint32_t q = ex[lg[s1] + 255u - lg[s0]];
  const uint32_t j = pt[kLocRatio + q];
  if (j == 0xffu) return kLocateUnexplained;
  const uint8_t* g = pt + kLocG + static_cast<size_t>(j) * kLocateRows;
  const uint32_t le = (lg[s0] + 255u - lg[g[0]]) % 255u;  // log of e = s_0 / G[0][j]
  bool ok = true;
  CALLFS_UNROLL
  for (int x = 2; x < NW * 4; ++x)
    if (x < rows) ok &= ex[lg[g[x]] + le] == locate_byte(s, x);
  return ok ? pt[kLocMap + j] : kLocateUnexplained;
}

struct LocateTables {
  // patterns, pat, sizes; one launch group (none when no stripe has a row) with its arena,
  // all-ones compare masks and r' per pattern in nrows; one tile map over the stripes with a
  // row; bytes = sum over them of size * (k + r')
  RaggedTables ragged;
  std::vector<uint8_t> gf;   // kLocGfBytes, shared by every pattern
  size_t stride = 0;         // locate_stride(k)
  std::vector<uint8_t> loc;  // [P][stride]
  // r' of pattern p (0: no row)
  uint32_t rows(size_t p) const {
    return ragged.mixed.groups.empty() ? 0u : ragged.mixed.groups[0].nrows[p];
  }
};

// present: batch * (k + m) flags. Errors and their order are build_ragged_tables'.
inline TableError build_locate_tables(int k, int m, int batch, const size_t* sizes,
                                      const uint8_t* present, LocateTables& t) {
  const int n = k + m;
  t = LocateTables();
  // nothing wanted: every row of every pattern is a compared one
  const std::vector<uint8_t> none(static_cast<size_t>(batch) * n, 0);
  const TableError e = build_ragged_tables(k, m, batch, sizes, present, none.data(), t.ragged);
  if (e != TableError::kOk) return e;
  MixedTables& mt = t.ragged.mixed;
  // the first launch group alone: compared shards past the 16th are not examined
  if (mt.groups.size() > 1) {
    mt.groups.resize(1);
    t.ragged.maps.resize(1);
  }
  mt.rows = mt.groups.empty() ? 0 : mt.groups[0].R;
  t.ragged.bytes = 0;
  for (int b = 0; b < batch; ++b) {
    const uint64_t r = t.rows(mt.pat[static_cast<size_t>(b)]);
    if (r == 0) continue;
    uint64_t add;
    if (__builtin_mul_overflow(static_cast<uint64_t>(sizes[b]), static_cast<uint64_t>(k) + r, &add) ||
        __builtin_add_overflow(t.ragged.bytes, add, &t.ragged.bytes))
      return TableError::kTooManyTiles;
  }
  const GF& g = gf();
  t.gf.assign(kLocGfBytes, 0);
  for (int i = 0; i < 256; ++i) t.gf[static_cast<size_t>(i)] = g.log[static_cast<size_t>(i)];
  for (int i = 0; i < 512; ++i) t.gf[256 + static_cast<size_t>(i)] = g.exp[static_cast<size_t>(i)];
  t.stride = locate_stride(k);
  const size_t P = mt.patterns.size();
  t.loc.assign(P * t.stride, 0);
  for (size_t p = 0; p < P; ++p) {
    const MixedPattern& pt = mt.patterns[p];
    uint8_t* blk = &t.loc[p * t.stride];
    const int rows = static_cast<int>(t.rows(p));
    for (size_t q = 0; q < 256; ++q) blk[kLocRatio + q] = 0xff;
    for (int j = 0; j < k; ++j) blk[kLocMap + static_cast<size_t>(j)] = static_cast<uint8_t>(pt.valid[static_cast<size_t>(j)]);
    for (int x = 0; x < rows; ++x)
      blk[kLocMap + static_cast<size_t>(k + x)] = static_cast<uint8_t>(pt.rows[static_cast<size_t>(x)]);
    if (rows == 0) continue;
    DecodePlan dp;
    if (!decode_plan(k, m, pt.mask.data(), none.data(), dp)) return TableError::kSingular;
    for (int j = 0; j < k; ++j)
      for (int x = 0; x < rows; ++x)
        blk[kLocG + static_cast<size_t>(j) * kLocateRows + static_cast<size_t>(x)] = dp.rows.at(x, j);
    if (rows < 2) continue;
    for (int j = 0; j < k; ++j) {
      const uint8_t q = g.mul[dp.rows.at(1, j)][g.inv(dp.rows.at(0, j))];
      blk[kLocRatio + q] = static_cast<uint8_t>(j);
    }
  }
  return TableError::kOk;
}

}  // namespace callfs
