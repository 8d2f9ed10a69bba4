// Host-side tables of locate plans and the classification rule on the CPU,
// built with g++ -fsanitize=address,undefined by tests/test_native_locate.py:
//  - per pattern, against decode_plan and a scalar shift-and-xor GF(2^8) multiply: the row
//    count r' = min(present - k, 16), G by column (no zero entry; G . valid = cmp on a
//    codeword), the ratio table (every position found, every other ratio 0xFF), the shard map;
//  - locate_classify, the function the kernel runs, exhaustively for RS(10,4), (4,2), (3,2),
//    (6,3), (1,3) and (20,12) with everything present and under seeded masks: every single
//    error (every examined position, every e = 1..255) is blamed on that shard, seeded columns
//    with 2..r'-1 errors are unexplained, r' = 1 is unexplained, no error is clean -- in every
//    packing width the kernel instances use;
//  - the tile map holds only the stripes with a row, a batch without one has no launch group,
//    and RS(10,20) with everything present uses 16 rows in one group;
//  - wide profiles, where positions and shard indices need all eight bits of the tables' bytes:
//    RS(129,9) and RS(240,16) with everything present (the latter examines exactly 256 shards)
//    and RS(240,16) with two data shards missing. Sampled: every examined position as the single
//    corrupt shard with a handful of error values, 1 and 0xFF among them, through locate_classify
//    and locate_correct (which must also return the position and the error value).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gf256.hpp"
#include "locate_tables.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// a * b in GF(2^8) mod 0x11D, no tables
uint8_t gmul(uint8_t a, uint8_t b) {
  unsigned r = 0, x = a;
  for (int i = 0; i < 8; ++i) {
    if ((b >> i) & 1u) r ^= x;
    x <<= 1;
    if (x & 0x100u) x ^= 0x11Du;
  }
  return static_cast<uint8_t>(r);
}
uint8_t ginv(uint8_t a) {
  for (int b = 1; b < 256; ++b)
    if (gmul(a, static_cast<uint8_t>(b)) == 1) return static_cast<uint8_t>(b);
  CHECK(false);
  return 0;
}

uint8_t g_mul[256][256];  // gmul, tabulated once

// The syndromes of one column, from the definition: stored cmp ^ G . valid.
std::vector<uint8_t> syndromes(const std::vector<uint8_t>& col, const std::vector<int>& valid,
                               const std::vector<int>& cmp, const Mat& G, int rows) {
  std::vector<uint8_t> s(static_cast<size_t>(rows));
  for (int x = 0; x < rows; ++x) {
    uint8_t v = col[static_cast<size_t>(cmp[static_cast<size_t>(x)])];
    for (size_t j = 0; j < valid.size(); ++j)
      v ^= g_mul[G.at(x, static_cast<int>(j))][col[static_cast<size_t>(valid[j])]];
    s[static_cast<size_t>(x)] = v;
  }
  return s;
}

template <int NW>
uint32_t classify(const std::vector<uint8_t>& s, int rows, int k, const uint8_t* gf, const uint8_t* pt) {
  uint32_t w[NW] = {0};
  // junk at and past `rows` must not be read
  for (int x = 0; x < NW * 4; ++x)
    w[x >> 2] |= static_cast<uint32_t>(x < rows ? s[static_cast<size_t>(x)] : 0xA5u) << (8 * (x & 3));
  return locate_classify(w, rows, k, gf, pt);
}

uint32_t classify_all(const std::vector<uint8_t>& s, int rows, int k, const uint8_t* gf, const uint8_t* pt) {
  const uint32_t v = classify<4>(s, rows, k, gf, pt);
  if (rows <= 8) CHECK(classify<2>(s, rows, k, gf, pt) == v);
  if (rows <= 4) CHECK(classify<1>(s, rows, k, gf, pt) == v);
  return v;
}

// locate_correct in the width NW: locate_classify's verdict for rows >= 3 (unexplained for
// every mismatch below), and for a shard verdict the position in valid then cmp and the value.
template <int NW>
void correct_one(const std::vector<uint8_t>& s, int rows, int k, const uint8_t* gf, const uint8_t* pt,
                 uint32_t verdict, uint32_t want_pos, uint32_t want_value) {
  uint32_t w[NW] = {0};
  for (int x = 0; x < NW * 4; ++x)
    w[x >> 2] |= static_cast<uint32_t>(x < rows ? s[static_cast<size_t>(x)] : 0xA5u) << (8 * (x & 3));
  uint32_t pos = 0xdeadu, value = 0xdeadu;
  const uint32_t v = locate_correct(w, rows, k, gf, pt, pos, value);
  if (rows < 3) {
    CHECK(v == (verdict == kLocateClean ? kLocateClean : kLocateUnexplained));
    return;
  }
  CHECK(v == verdict);
  if (v < 256u) CHECK(pos == want_pos && value == want_value);
}

void correct_all(const std::vector<uint8_t>& s, int rows, int k, const uint8_t* gf, const uint8_t* pt,
                 uint32_t verdict, uint32_t want_pos, uint32_t want_value) {
  correct_one<4>(s, rows, k, gf, pt, verdict, want_pos, want_value);
  if (rows <= 8) correct_one<2>(s, rows, k, gf, pt, verdict, want_pos, want_value);
  if (rows <= 4) correct_one<1>(s, rows, k, gf, pt, verdict, want_pos, want_value);
}

long g_singles = 0, g_multis = 0, g_wide_singles = 0;

// sampled: a handful of error values per position instead of all 255, and locate_correct too
void check_pattern(int k, int m, const LocateTables& t, size_t p, std::mt19937& rng, bool sampled = false) {
  const int n = k + m;
  const MixedPattern& pt = t.ragged.mixed.patterns[p];
  const uint8_t* blk = &t.loc[p * t.stride];
  const uint8_t* gf = t.gf.data();
  const std::vector<uint8_t> none(static_cast<size_t>(n), 0);
  DecodePlan dp;
  CHECK(decode_plan(k, m, pt.mask.data(), none.data(), dp));
  CHECK(dp.missing.empty());
  const int rows = static_cast<int>(t.rows(p));
  CHECK(rows == std::min<int>(static_cast<int>(dp.check.size()), kLocateRows));
  CHECK(pt.valid == dp.valid);
  // the shard map and G by column
  for (int j = 0; j < k; ++j) CHECK(blk[kLocMap + static_cast<size_t>(j)] == dp.valid[static_cast<size_t>(j)]);
  for (int x = 0; x < rows; ++x) CHECK(blk[kLocMap + static_cast<size_t>(k + x)] == dp.check[static_cast<size_t>(x)]);
  for (int j = 0; j < k; ++j)
    for (int x = 0; x < kLocateRows; ++x) {
      const uint8_t g = blk[kLocG + static_cast<size_t>(j) * kLocateRows + static_cast<size_t>(x)];
      if (x < rows) CHECK(g == dp.rows.at(x, j) && g != 0);
      else CHECK(g == 0);
    }
  // the ratio table
  int named = 0;
  for (int q = 0; q < 256; ++q) named += blk[kLocRatio + static_cast<size_t>(q)] != 0xff;
  if (rows >= 2) {
    CHECK(named == k);
    for (int j = 0; j < k; ++j)
      CHECK(blk[kLocRatio + gmul(dp.rows.at(1, j), ginv(dp.rows.at(0, j)))] == j);
  } else {
    CHECK(named == 0);
  }
  if (rows == 0) return;
  // a codeword column: E . data
  Mat E;
  CHECK(encode_matrix(k, m, E));
  std::vector<uint8_t> data(static_cast<size_t>(k)), col(static_cast<size_t>(n), 0);
  for (auto& d : data) d = static_cast<uint8_t>(rng());
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < k; ++j) col[static_cast<size_t>(i)] ^= gmul(E.at(i, j), data[static_cast<size_t>(j)]);
  std::vector<int> cmp(dp.check.begin(), dp.check.begin() + rows);
  std::vector<int> examined(dp.valid);
  examined.insert(examined.end(), cmp.begin(), cmp.end());
  // G . valid = cmp: a clean column is clean
  CHECK(classify_all(syndromes(col, dp.valid, cmp, dp.rows, rows), rows, k, gf, blk) == kLocateClean);
  // every single error
  static const int kSampled[] = {1, 2, 0x53, 0x80, 0xFE, 0xFF};
  for (size_t at = 0; at < examined.size(); ++at) {
    const int shard = examined[at];
    for (int q = 1; q < (sampled ? 1 + static_cast<int>(sizeof kSampled / sizeof kSampled[0]) : 256); ++q) {
      const int e = sampled ? kSampled[q - 1] : q;
      std::vector<uint8_t> bad(col);
      bad[static_cast<size_t>(shard)] ^= static_cast<uint8_t>(e);
      const std::vector<uint8_t> s = syndromes(bad, dp.valid, cmp, dp.rows, rows);
      const uint32_t v = classify_all(s, rows, k, gf, blk);
      CHECK(v == (rows < 2 ? kLocateUnexplained : static_cast<uint32_t>(shard)));
      ++g_singles;
      if (sampled) {
        correct_all(s, rows, k, gf, blk, v, static_cast<uint32_t>(at), static_cast<uint32_t>(e));
        ++g_wide_singles;
      }
    }
  }
  // junk in shards that are not examined changes nothing
  {
    std::vector<uint8_t> bad(col);
    for (int i = 0; i < n; ++i) {
      bool ex = false;
      for (int s : examined) ex |= s == i;
      if (!ex) bad[static_cast<size_t>(i)] ^= 0x5a;
    }
    CHECK(classify_all(syndromes(bad, dp.valid, cmp, dp.rows, rows), rows, k, gf, blk) == kLocateClean);
  }
  // 2 .. rows-1 errors: never blamed on anybody
  for (int c = 0; rows >= 3 && c < 300; ++c) {
    const int nerr = 2 + static_cast<int>(rng() % static_cast<unsigned>(rows - 2));
    std::vector<int> pos(examined);
    std::vector<uint8_t> bad(col);
    for (int q = 0; q < nerr; ++q) {
      const size_t at = static_cast<size_t>(q) + rng() % (pos.size() - static_cast<size_t>(q));
      std::swap(pos[static_cast<size_t>(q)], pos[at]);
      bad[static_cast<size_t>(pos[static_cast<size_t>(q)])] ^= static_cast<uint8_t>(1 + rng() % 255);
    }
    CHECK(classify_all(syndromes(bad, dp.valid, cmp, dp.rows, rows), rows, k, gf, blk) == kLocateUnexplained);
    ++g_multis;
  }
}

void profile(int k, int m, std::mt19937& rng) {
  const int n = k + m;
  // stripe 0 everything present, then seeded masks with k .. n shards present
  const int batch = 5;
  std::vector<uint8_t> pres(static_cast<size_t>(batch) * n, 1);
  std::vector<size_t> sizes(static_cast<size_t>(batch));
  for (int b = 0; b < batch; ++b) sizes[static_cast<size_t>(b)] = 1 + rng() % 40000;
  for (int b = 1; b < batch; ++b) {
    const int drop = b == 1 ? m : static_cast<int>(rng() % static_cast<unsigned>(m));  // b = 1: no row
    for (int d = 0; d < drop;) {
      const size_t i = rng() % static_cast<unsigned>(n);
      if (!pres[static_cast<size_t>(b) * n + i]) continue;
      pres[static_cast<size_t>(b) * n + i] = 0;
      ++d;
    }
  }
  LocateTables t;
  CHECK(build_locate_tables(k, m, batch, sizes.data(), pres.data(), t) == TableError::kOk);
  const MixedTables& mt = t.ragged.mixed;
  CHECK(mt.groups.size() == 1 && t.ragged.maps.size() == 1);
  CHECK(t.gf.size() == kLocGfBytes && t.stride == locate_stride(k) && t.loc.size() == t.stride * mt.patterns.size());
  for (int a = 1; a < 256; ++a) {
    CHECK(t.gf[256 + t.gf[static_cast<size_t>(a)]] == a);  // exp[log[a]] = a
    CHECK(t.gf[256 + 255 + t.gf[static_cast<size_t>(a)]] == a);
  }
  CHECK(t.gf[256 + 1] == 2 && gmul(t.gf[256 + 7], 2) == t.gf[256 + 8]);
  // the tile map: the stripes with a row alone; bytes = sum of size * (k + r')
  const TileMap& tm = t.ragged.maps[0];
  uint64_t bytes = 0, tiles = 0;
  int with_row = 0;
  for (int b = 0; b < batch; ++b) {
    const uint32_t r = t.rows(mt.pat[static_cast<size_t>(b)]);
    if (b == 1) CHECK(r == 0);
    if (r == 0) continue;
    ++with_row;
    bytes += sizes[static_cast<size_t>(b)] * (static_cast<uint64_t>(k) + r);
    CHECK(tm.tile0[static_cast<size_t>(b)] == tiles);
    tiles += ragged_tiles(sizes[static_cast<size_t>(b)]);
    CHECK(mt.groups[0].vmask[mt.pat[static_cast<size_t>(b)]] == (r == 32 ? ~0u : (1u << r) - 1u));
  }
  CHECK(tm.stripes == with_row && tm.ntiles == tiles && t.ragged.bytes == bytes);
  for (uint32_t s : tm.tile_stripe) CHECK(s != 1u && t.rows(mt.pat[s]) != 0);
  for (size_t p = 0; p < mt.patterns.size(); ++p) check_pattern(k, m, t, p, rng);
}

// A wide profile: stripe 0 with everything present and, when `lost` names shards, stripe 1
// without them. Every pattern's tables and the sampled rule.
void wide_profile(int k, int m, const std::vector<int>& lost, int want_rows_lost, std::mt19937& rng) {
  const int n = k + m, batch = lost.empty() ? 1 : 2;
  std::vector<uint8_t> pres(static_cast<size_t>(batch) * n, 1);
  for (int i : lost) pres[static_cast<size_t>(n + i)] = 0;
  const std::vector<size_t> sizes(static_cast<size_t>(batch), 8211);
  LocateTables t;
  CHECK(build_locate_tables(k, m, batch, sizes.data(), pres.data(), t) == TableError::kOk);
  const MixedTables& mt = t.ragged.mixed;
  CHECK(mt.groups.size() == 1 && mt.patterns.size() == static_cast<size_t>(batch));
  CHECK(t.stride == locate_stride(k) && t.loc.size() == t.stride * mt.patterns.size());
  CHECK(static_cast<int>(t.rows(mt.pat[0])) == std::min(m, kLocateRows));
  if (batch > 1) CHECK(static_cast<int>(t.rows(mt.pat[1])) == want_rows_lost);
  for (size_t p = 0; p < mt.patterns.size(); ++p) check_pattern(k, m, t, p, rng, true);
}

}  // namespace

int main() {
  for (int a = 0; a < 256; ++a)
    for (int b = 0; b < 256; ++b) g_mul[a][b] = gmul(static_cast<uint8_t>(a), static_cast<uint8_t>(b));
  std::mt19937 rng(20261020);
  const int profiles[][2] = {{10, 4}, {4, 2}, {3, 2}, {6, 3}, {1, 3}, {20, 12}};
  for (const auto& pr : profiles) profile(pr[0], pr[1], rng);
  {  // RS(10,20), everything present: 16 of the 20 compared shards, one launch group
    const int k = 10, m = 20, n = 30;
    std::vector<uint8_t> pres(static_cast<size_t>(2 * n), 1);
    const size_t sizes[2] = {100, 9000};
    LocateTables t;
    CHECK(build_locate_tables(k, m, 2, sizes, pres.data(), t) == TableError::kOk);
    CHECK(t.ragged.mixed.groups.size() == 1 && t.ragged.mixed.groups[0].R == 16);
    CHECK(t.ragged.mixed.patterns.size() == 1 && t.rows(0) == 16);
    CHECK(t.ragged.bytes == (100u + 9000u) * 26u);
    check_pattern(k, m, t, 0, rng);
    // the 4 shards past the 16th compared one are in no table
    const uint8_t* blk = t.loc.data();
    for (int x = 0; x < 16; ++x) CHECK(blk[kLocMap + 10 + static_cast<size_t>(x)] == 10 + x);
  }
  {  // exactly k present everywhere: no row, no launch group, no tile
    const int k = 4, m = 2, n = 6;
    std::vector<uint8_t> pres(static_cast<size_t>(2 * n), 1);
    pres[0] = pres[5] = pres[6 + 2] = pres[6 + 3] = 0;
    const size_t sizes[2] = {17, 8193};
    LocateTables t;
    CHECK(build_locate_tables(k, m, 2, sizes, pres.data(), t) == TableError::kOk);
    CHECK(t.ragged.mixed.groups.empty() && t.ragged.bytes == 0 && t.rows(0) == 0);
  }
  {  // errors are build_ragged_tables'
    const int k = 4, m = 2, n = 6;
    std::vector<uint8_t> pres(static_cast<size_t>(n), 1);
    size_t zero = 0, one = 1;
    LocateTables t;
    CHECK(build_locate_tables(k, m, 1, &zero, pres.data(), t) == TableError::kNoData);
    pres[0] = pres[1] = pres[2] = 0;
    CHECK(build_locate_tables(k, m, 1, &one, pres.data(), t) == TableError::kTooFewShards);
  }
  // positions and shard indices at and past 128, and the 256 examined shards of RS(240,16)
  wide_profile(129, 9, {}, 0, rng);
  wide_profile(240, 16, {1, 128}, 14, rng);
  CHECK(g_wide_singles == 6L * (138 + 256 + 254));
  std::printf("singles %ld multis %ld wide singles %ld\nlocate_host_test ok\n", g_singles, g_multis,
              g_wide_singles);
  return 0;
}
