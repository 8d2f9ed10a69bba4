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
// A pair plan (max_errors = 2) appends what locate_classify2 reads to name
// two corrupt shards per column: the power-syndrome matrix H_cmp, the point -> position table
// and, in the shared block, the roots of z^2 + z = c.
// A correct plan has a locate plan's tables (max_errors = 1) and runs
// locate_correct, which also says where and what to XOR to repair a single error.
// Plain C++ with no HIP dependence (tests/native/locate_host_test.cpp, locate2_host_test.cpp and
// correct_host_test.cpp build it with g++ on the CPU); locate_classify, locate_classify2 and
// locate_correct are the functions the kernels and the CPU tests both run.
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
// A pair plan's verdict for a column with two corrupt shards a < b: above every shard index,
// below both sentinels.
constexpr uint32_t kLocatePair = 0x10000u;
CALLFS_HD inline uint32_t locate_pair(uint32_t a, uint32_t b) {
  return kLocatePair | (a < b ? (a << 8) | b : (b << 8) | a);
}
CALLFS_HD inline bool locate_is_pair(uint32_t v) { return (v >> 16) == 1u; }

// One pattern's block of the device tables, kLocStride(k) bytes:
constexpr size_t kLocRatio = 0;        // [256] ratio -> position in valid, 0xFF = none
constexpr size_t kLocMap = 256;        // [k + 16] position -> shard index: valid, then cmp
constexpr size_t kLocG = 256 + 272;    // [k][16] G by column: G[x][j] at j * 16 + x
CALLFS_HD inline size_t locate_stride(int k) { return kLocG + static_cast<size_t>(k) * kLocateRows; }
// A pair plan's block is that block and, behind it (at locate_stride(k) + ...):
constexpr size_t kLoc2H = 0;        // [16][16] H_cmp by row: H[i][x] at i * 16 + x, 0 past r'
constexpr size_t kLoc2Point = 256;  // [256] point -> position in valid then cmp, 0xFF = none
constexpr size_t kLoc2Bytes = 512;  // (the rule asks only whether a point has a position: shard
                                    // i sits at point i; position 255 of a pattern that
                                    // examines 256 shards is stored as 0xFE)
inline size_t locate_stride(int k, int max_errors) {
  return locate_stride(k) + (max_errors > 1 ? kLoc2Bytes : 0);
}
// The block every pattern shares: log[256], then exp[512] (exp[i] = 2^(i mod 255))
constexpr size_t kLocGfBytes = 768;
// A pair plan's shared block adds [256] c -> the even root z of z^2 + z = c, 0xFF = no root
// (the other root is z ^ 1; 0xFF is odd, so no stored root equals it)
constexpr size_t kLoc2Z = 768;
constexpr size_t kLoc2GfBytes = 1024;

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

// The correction of one byte column (correct plans): locate_classify's
// decision for a single error, and with a shard verdict where and what to XOR: `pos`, the
// shard's position in T = valid then cmp (j for valid[j], k + x for cmp[x]), and `value`, the
// error e = s_0 / G[0][j] (or s_x). A column is corrected only when rows >= 3: the verdict
// takes two syndromes and at least one further row must confirm it -- a corrected column is a
// codeword by construction, so nothing after the write could catch a miscorrection. With
// rows < 3 every mismatching column is unexplained. For rows >= 3 the verdict is
// locate_classify's: one corrupt byte is restored exactly, 2..rows-1 are left alone.
// (The decision is written out again, not shared with locate_classify: the locate kernels'
// code stays what it was, instruction for instruction.)
template <int NW>
CALLFS_HD inline uint32_t locate_correct(const uint32_t (&s)[NW], int rows, int k, const uint8_t* gf,
                                         const uint8_t* pt, uint32_t& pos, uint32_t& value) {
  int nz = 0, first = 0;
  CALLFS_UNROLL
  for (int x = NW * 4 - 1; x >= 0; --x) {
    if (x < rows && locate_byte(s, x) != 0) {
      ++nz;
      first = x;
    }
  }
  if (nz == 0) return kLocateClean;
  if (rows < 3) return kLocateUnexplained;
  if (nz == 1) {
    uint32_t sx = 0;
    CALLFS_UNROLL
    for (int x = 0; x < NW * 4; ++x) sx |= x < rows ? locate_byte(s, x) : 0u;  // the others are zero
    pos = static_cast<uint32_t>(k + first);
    value = sx;
    return pt[kLocMap + static_cast<size_t>(k) + first];
  }
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
  if (!ok) return kLocateUnexplained;
  pos = j;
  value = ex[le];
  return pt[kLocMap + j];
}

// a . b and a / b (b != 0) from the shared log / exp block
CALLFS_HD inline uint32_t locate_mul(const uint8_t* gf, uint32_t a, uint32_t b) {
  return a && b ? gf[256 + gf[a] + gf[b]] : 0u;
}
CALLFS_HD inline uint32_t locate_div(const uint8_t* gf, uint32_t a, uint32_t b) {
  return a ? gf[256 + gf[a] + 255u - gf[b]] : 0u;
}

// Power syndrome S_i = sum over x < rows of H_cmp[i][x] . s_x, h = row i of H_cmp.
template <int NW>
CALLFS_HD inline uint32_t locate_power(const uint32_t (&s)[NW], int rows, const uint8_t* gf, const uint8_t* h) {
  uint32_t acc = 0;
  CALLFS_UNROLL
  for (int x = 0; x < NW * 4; ++x)
    if (x < rows) acc ^= locate_mul(gf, h[x], locate_byte(s, x));
  return acc;
}

#if defined(__clang__)
#define CALLFS_NO_UNROLL _Pragma("unroll 1")
#else
#define CALLFS_NO_UNROLL
#endif

// The pair rule for a column locate_classify left unexplained in a pattern
// that compares rows >= 4 shards: the column is tried as two errors at points X_a != X_b of the
// rows x (k + rows) generalised RS code whose power syndromes are S = H_cmp . s. The locator
// x^2 + sigma1 x + sigma2 comes from S_0..S_3; every further recurrence S_i = sigma1 S_{i-1} +
// sigma2 S_{i-2} must hold; its roots come through z^2 + z = sigma2 / sigma1^2; both must be
// points of examined shards and both error terms nonzero. Returns locate_pair(X_a, X_b) (shard
// i sits at point i), else unexplained. gf: the pair plan's shared block (kLoc2GfBytes); pt:
// the pattern's block, the single rule's locate_stride(k) bytes and the pair tables behind.
// The loops over i stay loops (one unrolled pass over the rows each) and S_i are formed one
// at a time: the kernel holds one copy of this per call site, and a handful of registers.
template <int NW>
CALLFS_HD inline uint32_t locate_pair_rule(const uint32_t (&s)[NW], int rows, int k,
                                           const uint8_t* gf, const uint8_t* pt) {
  const uint8_t* h = pt + locate_stride(k) + kLoc2H;
  const uint8_t* point = pt + locate_stride(k) + kLoc2Point;
  uint32_t S0 = 0, S1 = 0, Sa = 0, Sb = 0;  // Sa, Sb: S_2, S_3, then the last two formed
  CALLFS_NO_UNROLL
  for (int i = 0; i < 4; ++i) {
    const uint32_t Si = locate_power(s, rows, gf, h + 16 * i);
    S0 = i == 0 ? Si : S0;
    S1 = i == 1 ? Si : S1;
    Sa = i == 2 ? Si : Sa;
    Sb = i == 3 ? Si : Sb;
  }
  const uint32_t det = locate_mul(gf, S1, S1) ^ locate_mul(gf, S0, Sa);
  if (det == 0) return kLocateUnexplained;
  const uint32_t sg1 = locate_div(gf, locate_mul(gf, S1, Sa) ^ locate_mul(gf, S0, Sb), det);
  const uint32_t sg2 = locate_div(gf, locate_mul(gf, S1, Sb) ^ locate_mul(gf, Sa, Sa), det);
  bool ok = true;
  CALLFS_NO_UNROLL
  for (int i = 4; i < rows; ++i) {
    const uint32_t Si = locate_power(s, rows, gf, h + 16 * i);
    ok &= Si == (locate_mul(gf, sg1, Sb) ^ locate_mul(gf, sg2, Sa));
    Sa = Sb;
    Sb = Si;
  }
  if (!ok || sg1 == 0) return kLocateUnexplained;
  const uint32_t z = gf[kLoc2Z + locate_div(gf, sg2, locate_mul(gf, sg1, sg1))];
  if (z == 0xffu) return kLocateUnexplained;
  const uint32_t Xa = locate_mul(gf, sg1, z), Xb = Xa ^ sg1;
  if (point[Xa] == 0xffu || point[Xb] == 0xffu) return kLocateUnexplained;
  // u_a e_a = (S_1 + S_0 X_b) / (X_a + X_b) and u_b e_b = S_0 + that; X_a + X_b = sigma1
  const uint32_t ea = locate_div(gf, S1 ^ locate_mul(gf, S0, Xb), sg1);
  if (ea == 0 || (S0 ^ ea) == 0) return kLocateUnexplained;
  return locate_pair(Xa, Xb);
}

// The verdict of one byte column of a pair plan: locate_classify's, unless that is
// "unexplained" and rows >= 4; then locate_pair_rule's.
template <int NW>
CALLFS_HD inline uint32_t locate_classify2(const uint32_t (&s)[NW], int rows, int k,
                                           const uint8_t* gf, const uint8_t* pt) {
  const uint32_t v = locate_classify(s, rows, k, gf, pt);
  return v == kLocateUnexplained && rows >= 4 ? locate_pair_rule(s, rows, k, gf, pt) : v;
}

struct LocateTables {
  // patterns, pat, sizes; one launch group (none when no stripe has a row) with its arena,
  // all-ones compare masks and r' per pattern in nrows; one tile map over the stripes with a
  // row; bytes = sum over them of size * (k + r')
  RaggedTables ragged;
  int max_errors = 1;        // 2: a pair plan
  std::vector<uint8_t> gf;   // kLocGfBytes (kLoc2GfBytes for a pair plan), shared by every pattern
  size_t stride = 0;         // locate_stride(k, max_errors)
  std::vector<uint8_t> loc;  // [P][stride]
  // r' of pattern p (0: no row)
  uint32_t rows(size_t p) const {
    return ragged.mixed.groups.empty() ? 0u : ragged.mixed.groups[0].nrows[p];
  }
};

// present: batch * (k + m) flags. Errors and their order are build_ragged_tables'. max_errors
// 1 or 2 (the caller checks): 2 appends the pair tables, and changes nothing before them.
inline TableError build_locate_tables(int k, int m, int batch, const size_t* sizes,
                                      const uint8_t* present, LocateTables& t, int max_errors = 1) {
  const int n = k + m;
  t = LocateTables();
  t.max_errors = max_errors;
  const bool pair = max_errors > 1;
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
  t.gf.assign(pair ? kLoc2GfBytes : kLocGfBytes, 0);
  for (int i = 0; i < 256; ++i) t.gf[static_cast<size_t>(i)] = g.log[static_cast<size_t>(i)];
  for (int i = 0; i < 512; ++i) t.gf[256 + static_cast<size_t>(i)] = g.exp[static_cast<size_t>(i)];
  if (pair) {
    for (size_t c = 0; c < 256; ++c) t.gf[kLoc2Z + c] = 0xff;
    for (unsigned z = 0; z < 256; z += 2) t.gf[kLoc2Z + (g.mul[z][z] ^ z)] = static_cast<uint8_t>(z);
  }
  t.stride = locate_stride(k, max_errors);
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
    if (pair) {
      // the examined shards T = valid then cmp; shard i sits at the point i
      std::vector<int> T(pt.valid.begin(), pt.valid.begin() + k);
      T.insert(T.end(), pt.rows.begin(), pt.rows.begin() + rows);
      uint8_t* b2 = blk + locate_stride(k);
      for (size_t x = 0; x < 256; ++x) b2[kLoc2Point + x] = 0xff;
      for (size_t j = 0; j < T.size(); ++j)
        b2[kLoc2Point + static_cast<size_t>(T[j])] = static_cast<uint8_t>(j < 0xfe ? j : 0xfe);
      // H_cmp[i][x] = u . a^i, a the point of cmp[x], u = 1 / prod over the other l in T of (a + l)
      for (int x = 0; x < rows; ++x) {
        const uint8_t a = static_cast<uint8_t>(pt.rows[static_cast<size_t>(x)]);
        uint8_t prod = 1;
        for (int l : T)
          if (l != a) prod = g.mul[prod][a ^ static_cast<uint8_t>(l)];
        const uint8_t u = g.inv(prod);
        for (int i = 0; i < rows; ++i)
          b2[kLoc2H + static_cast<size_t>(i) * kLocateRows + static_cast<size_t>(x)] = g.mul[u][g.pow(a, i)];
      }
    }
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
