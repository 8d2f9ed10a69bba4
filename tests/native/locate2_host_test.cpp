// The pair rule of locate plans (locate_classify2 and the tables
// build_locate_tables appends for max_errors = 2) on the CPU, built with g++
// -fsanitize=address,undefined by tests/test_native_locate2.py. Against a scalar shift-and-xor
// GF(2^8) multiply and syndromes formed from their definition:
//  - tables: with max_errors = 1 they are byte for byte what build_locate_tables builds without
//    the argument, and a pair plan's blocks begin with exactly those bytes; H_cmp . s equals
//    H . y from the definition of H on random columns; the point table names the examined
//    shards and nothing else; the z-table is exact for all 256 c;
//  - every single error (every examined position, every e = 1..255) gets locate_classify's
//    verdict;
//  - RS(10,4) with everything present: every pair of examined positions x every (e_a, e_b),
//    91 x 255^2 columns, is blamed on exactly that pair;
//  - RS(1,4), (6,4), (16,4), (4,5), (10,8), (20,12) and (10,20) (16 rows), everything present
//    and under seeded masks that leave r' >= 4: seeded pairs, pairs with shard 0 among them,
//    are blamed on exactly the pair; seeded columns with 3..r'-2 errors are unexplained;
//  - patterns with r' <= 3: the verdict is locate_classify's on seeded 1- and 2-error columns;
//  - wide profiles, where positions and points need all eight bits of the tables' bytes:
//    RS(129,9) and RS(240,16) with everything present (256 examined shards: position 255 has its
//    own encoding in the point table) and RS(240,16) with two data shards missing, sampled: every
//    examined position as the single corrupt shard with a handful of values, every pair drawn
//    from the positions {0, 1, 127, 128, k-1, k, 254, 255} with a few value pairs, seeded pairs
//    and seeded 3..r'-2 errors;
// all in every packing width the kernel instances use.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
uint8_t gpow(uint8_t a, int n) {  // 0^0 = 1
  uint8_t r = 1;
  for (int i = 0; i < n; ++i) r = gmul(r, a);
  return r;
}

uint8_t g_mul[256][256];  // gmul, tabulated once

template <int NW>
void pack(const uint8_t* s, int rows, uint32_t (&w)[NW]) {
  // junk at and past `rows` must not be read
  for (int i = 0; i < NW; ++i) w[i] = 0;
  for (int x = 0; x < NW * 4; ++x)
    w[x >> 2] |= static_cast<uint32_t>(x < rows ? s[x] : 0xA5u) << (8 * (x & 3));
}

template <int NW>
uint32_t classify2(const uint8_t* s, int rows, int k, const uint8_t* gf, const uint8_t* pt) {
  uint32_t w[NW];
  pack(s, rows, w);
  return locate_classify2(w, rows, k, gf, pt);
}
template <int NW>
uint32_t classify1(const uint8_t* s, int rows, int k, const uint8_t* gf, const uint8_t* pt) {
  uint32_t w[NW];
  pack(s, rows, w);
  return locate_classify(w, rows, k, gf, pt);
}

// locate_classify2 in every width that holds `rows`; the widths must agree
uint32_t classify2_all(const uint8_t* s, int rows, int k, const uint8_t* gf, const uint8_t* pt) {
  const uint32_t v = classify2<4>(s, rows, k, gf, pt);
  if (rows <= 8) CHECK(classify2<2>(s, rows, k, gf, pt) == v);
  if (rows <= 4) CHECK(classify2<1>(s, rows, k, gf, pt) == v);
  return v;
}
uint32_t classify1_all(const uint8_t* s, int rows, int k, const uint8_t* gf, const uint8_t* pt) {
  const uint32_t v = classify1<4>(s, rows, k, gf, pt);
  if (rows <= 8) CHECK(classify1<2>(s, rows, k, gf, pt) == v);
  if (rows <= 4) CHECK(classify1<1>(s, rows, k, gf, pt) == v);
  return v;
}

// One pattern of a pair plan: T = valid then cmp, and unit[j] = the syndromes (from their
// definition s_x = stored cmp[x] ^ G[x] . valid) of an error of value 1 at position j of T.
struct Pattern {
  int k = 0, rows = 0;
  std::vector<int> T;
  std::vector<std::vector<uint8_t>> unit;
  const uint8_t* gf = nullptr;
  const uint8_t* blk = nullptr;
};

Pattern make_pattern(int k, int m, const LocateTables& t, size_t p) {
  const int n = k + m;
  const MixedPattern& mp = t.ragged.mixed.patterns[p];
  Pattern P;
  P.k = k;
  P.rows = static_cast<int>(t.rows(p));
  P.gf = t.gf.data();
  P.blk = &t.loc[p * t.stride];
  const std::vector<uint8_t> none(static_cast<size_t>(n), 0);
  DecodePlan dp;
  CHECK(decode_plan(k, m, mp.mask.data(), none.data(), dp));
  P.T = dp.valid;
  P.T.insert(P.T.end(), dp.check.begin(), dp.check.begin() + P.rows);
  for (size_t j = 0; j < P.T.size(); ++j) {
    std::vector<uint8_t> s(16, 0);
    for (int x = 0; x < P.rows; ++x)
      s[static_cast<size_t>(x)] = j < static_cast<size_t>(k) ? dp.rows.at(x, static_cast<int>(j))
                                                               : (static_cast<int>(j) - k == x ? 1 : 0);
    P.unit.push_back(s);
  }
  return P;
}

// The syndromes of errors e[q] at positions pos[q] of T (the code is linear: a codeword adds 0).
void syndromes(const Pattern& P, const int* pos, const uint8_t* e, int nerr, uint8_t* s) {
  std::memset(s, 0, 16);
  for (int q = 0; q < nerr; ++q) {
    const uint8_t* u = P.unit[static_cast<size_t>(pos[q])].data();
    for (int x = 0; x < P.rows; ++x) s[x] ^= g_mul[u[x]][e[q]];
  }
}

long g_singles = 0, g_pairs = 0, g_multis = 0, g_short = 0;

void check_tables(int k, const LocateTables& t, const LocateTables& t1, size_t p, const Pattern& P,
                  std::mt19937& rng) {
  const size_t s1 = locate_stride(k);
  CHECK(t.stride == s1 + kLoc2Bytes && t1.stride == s1);
  // the single rule's bytes are untouched
  CHECK(std::memcmp(&t.loc[p * t.stride], &t1.loc[p * t1.stride], s1) == 0);
  const uint8_t* b2 = P.blk + s1;
  // the point table: the examined shards, at their positions
  int named = 0;
  for (int x = 0; x < 256; ++x) named += b2[kLoc2Point + static_cast<size_t>(x)] != 0xff;
  CHECK(named == static_cast<int>(P.T.size()));
  for (size_t j = 0; j < P.T.size(); ++j)
    CHECK(b2[kLoc2Point + static_cast<size_t>(P.T[j])] == std::min<size_t>(j, 0xfe));
  // H from its definition: H[i][j] = u_j . a_j^i, u_j = 1 / prod over l != j of (a_j + a_l)
  const int rows = P.rows, nT = static_cast<int>(P.T.size());
  std::vector<uint8_t> u(static_cast<size_t>(nT));
  for (int j = 0; j < nT; ++j) {
    uint8_t prod = 1;
    for (int l = 0; l < nT; ++l)
      if (l != j) prod = gmul(prod, static_cast<uint8_t>(P.T[static_cast<size_t>(j)] ^ P.T[static_cast<size_t>(l)]));
    CHECK(prod != 0);
    u[static_cast<size_t>(j)] = ginv(prod);
  }
  for (int i = 0; i < 16; ++i)
    for (int x = 0; x < 16; ++x) {
      const uint8_t h = b2[kLoc2H + static_cast<size_t>(i) * 16 + static_cast<size_t>(x)];
      if (i < rows && x < rows)
        CHECK(h == gmul(u[static_cast<size_t>(k + x)], gpow(static_cast<uint8_t>(P.T[static_cast<size_t>(k + x)]), i)));
      else
        CHECK(h == 0);
    }
  // H_cmp . s = H . y on random columns (y = the error over T: H . codeword = 0)
  for (int c = 0; c < 20 && rows > 0; ++c) {
    std::vector<int> pos(static_cast<size_t>(nT));
    std::vector<uint8_t> y(static_cast<size_t>(nT));
    for (int j = 0; j < nT; ++j) {
      pos[static_cast<size_t>(j)] = j;
      y[static_cast<size_t>(j)] = static_cast<uint8_t>(rng());
    }
    uint8_t s[16];
    syndromes(P, pos.data(), y.data(), nT, s);
    for (int i = 0; i < rows; ++i) {
      uint8_t want = 0, got = 0;
      for (int j = 0; j < nT; ++j)
        want ^= gmul(gmul(u[static_cast<size_t>(j)], gpow(static_cast<uint8_t>(P.T[static_cast<size_t>(j)]), i)), y[static_cast<size_t>(j)]);
      for (int x = 0; x < rows; ++x) got ^= gmul(b2[kLoc2H + static_cast<size_t>(i) * 16 + static_cast<size_t>(x)], s[x]);
      CHECK(want == got);
      uint32_t w[4];
      pack(s, rows, w);
      CHECK(locate_power(w, rows, P.gf, b2 + kLoc2H + 16 * static_cast<size_t>(i)) == want);
    }
  }
}

void check_singles(const Pattern& P) {
  uint8_t s[16];
  for (int j = 0; j < static_cast<int>(P.T.size()); ++j)
    for (int e = 1; e < 256; ++e) {
      const uint8_t ev = static_cast<uint8_t>(e);
      syndromes(P, &j, &ev, 1, s);
      const uint32_t v1 = classify1_all(s, P.rows, P.k, P.gf, P.blk);
      CHECK(classify2_all(s, P.rows, P.k, P.gf, P.blk) == v1);
      if (P.rows >= 2) CHECK(v1 == static_cast<uint32_t>(P.T[static_cast<size_t>(j)]));
      ++g_singles;
    }
  std::memset(s, 0, sizeof s);
  CHECK(classify2_all(s, P.rows, P.k, P.gf, P.blk) == kLocateClean);
}

uint32_t pair_of(const Pattern& P, int a, int b) {
  return locate_pair(static_cast<uint32_t>(P.T[static_cast<size_t>(a)]), static_cast<uint32_t>(P.T[static_cast<size_t>(b)]));
}

void check_pair(const Pattern& P, int a, int b, uint8_t ea, uint8_t eb) {
  const int pos[2] = {a, b};
  const uint8_t e[2] = {ea, eb};
  uint8_t s[16];
  syndromes(P, pos, e, 2, s);
  const uint32_t v = classify2_all(s, P.rows, P.k, P.gf, P.blk);
  if (P.rows >= 4) {
    CHECK(v == pair_of(P, a, b));
    CHECK(locate_is_pair(v) && v != kLocateClean && v != kLocateUnexplained && v > 0xffu);
    ++g_pairs;
  } else {
    CHECK(v == classify1_all(s, P.rows, P.k, P.gf, P.blk));
    ++g_short;
  }
}

// seeded pairs, pairs that hold position 0 (shard 0 when it is present) among them; then
// 3..rows-2 errors
void check_seeded(const Pattern& P, std::mt19937& rng) {
  const int nT = static_cast<int>(P.T.size());
  for (int c = 0; c < 400; ++c) {
    int a = c % 5 == 0 ? 0 : static_cast<int>(rng() % static_cast<unsigned>(nT));
    int b = static_cast<int>(rng() % static_cast<unsigned>(nT - 1));
    if (b >= a) ++b;
    check_pair(P, a, b, static_cast<uint8_t>(1 + rng() % 255), static_cast<uint8_t>(1 + rng() % 255));
  }
  for (int c = 0; P.rows >= 5 && c < 300; ++c) {
    const int nerr = 3 + static_cast<int>(rng() % static_cast<unsigned>(P.rows - 4));  // 3..rows-2
    std::vector<int> pos(static_cast<size_t>(nT));
    for (int j = 0; j < nT; ++j) pos[static_cast<size_t>(j)] = j;
    uint8_t e[16];
    for (int q = 0; q < nerr; ++q) {
      std::swap(pos[static_cast<size_t>(q)], pos[static_cast<size_t>(q) + rng() % static_cast<unsigned>(nT - q)]);
      e[q] = static_cast<uint8_t>(1 + rng() % 255);
    }
    uint8_t s[16];
    syndromes(P, pos.data(), e, nerr, s);
    CHECK(classify2_all(s, P.rows, P.k, P.gf, P.blk) == kLocateUnexplained);
    ++g_multis;
  }
}

// Stripe 0 with everything present, then `masks` seeded stripes that keep at least k + keep
// shards (keep = 4: r' >= 4; keep = 1 with drop forced: r' <= 3).
void profile(int k, int m, bool short_rows, std::mt19937& rng) {
  const int n = k + m, batch = 4;
  std::vector<uint8_t> pres(static_cast<size_t>(batch) * n, 1);
  std::vector<size_t> sizes(static_cast<size_t>(batch), 64);
  for (int b = 1; b < batch; ++b) {
    int drop;
    if (short_rows) drop = m - (1 + (b - 1) % std::min(3, m));  // r' = 1, 2, 3
    else drop = m > 4 ? static_cast<int>(rng() % static_cast<unsigned>(m - 3)) : 0;  // r' >= 4
    int d = 0;
    if (b == 1 && !short_rows && m > 4) {  // shard 0 missing: the point 0 is outside T
      drop = std::max(drop, 1);
      pres[static_cast<size_t>(b) * n] = 0;
      d = 1;
    }
    while (d < drop) {
      const size_t i = rng() % static_cast<unsigned>(n);
      if (!pres[static_cast<size_t>(b) * n + i]) continue;
      pres[static_cast<size_t>(b) * n + i] = 0;
      ++d;
    }
  }
  LocateTables t, t1, t0;
  CHECK(build_locate_tables(k, m, batch, sizes.data(), pres.data(), t, 2) == TableError::kOk);
  CHECK(build_locate_tables(k, m, batch, sizes.data(), pres.data(), t1, 1) == TableError::kOk);
  CHECK(build_locate_tables(k, m, batch, sizes.data(), pres.data(), t0) == TableError::kOk);
  // max_errors = 1: exactly the tables of the call without it
  CHECK(t1.gf == t0.gf && t1.loc == t0.loc && t1.stride == t0.stride && t1.max_errors == 1);
  CHECK(t1.gf.size() == kLocGfBytes && t1.stride == locate_stride(k));
  CHECK(t1.ragged.bytes == t0.ragged.bytes && t.ragged.bytes == t0.ragged.bytes);
  CHECK(t.max_errors == 2 && t.gf.size() == kLoc2GfBytes);
  CHECK(std::memcmp(t.gf.data(), t1.gf.data(), kLocGfBytes) == 0);
  const size_t P = t.ragged.mixed.patterns.size();
  CHECK(t1.ragged.mixed.patterns.size() == P && t.loc.size() == P * t.stride);
  for (size_t p = 0; p < P; ++p) {
    const Pattern pt = make_pattern(k, m, t, p);
    CHECK(short_rows || p == 0 || pt.rows >= 4);
    check_tables(k, t, t1, p, pt, rng);
    if (pt.rows == 0) continue;
    check_singles(pt);
    check_seeded(pt, rng);
  }
}

long g_wide_singles = 0, g_wide_pairs = 0;

// A wide profile, where positions and points need all eight bits of the tables' bytes: stripe 0
// with everything present and, when `lost` names shards, stripe 1 without them. Sampled: every
// examined position as the single corrupt shard with a handful of error values, and every pair
// of the positions {0, 1, 127, 128, k-1, k, 254, 255} that the pattern has, with a few value
// pairs.
void wide_profile(int k, int m, const std::vector<int>& lost, std::mt19937& rng) {
  const int n = k + m, batch = lost.empty() ? 1 : 2;
  std::vector<uint8_t> pres(static_cast<size_t>(batch) * n, 1);
  for (int i : lost) pres[static_cast<size_t>(n + i)] = 0;
  const std::vector<size_t> sizes(static_cast<size_t>(batch), 8211);
  LocateTables t, t1;
  CHECK(build_locate_tables(k, m, batch, sizes.data(), pres.data(), t, 2) == TableError::kOk);
  CHECK(build_locate_tables(k, m, batch, sizes.data(), pres.data(), t1, 1) == TableError::kOk);
  CHECK(t.ragged.mixed.patterns.size() == static_cast<size_t>(batch));
  static const uint8_t kValues[] = {1, 2, 0x53, 0x80, 0xFE, 0xFF};
  static const uint8_t kValuePairs[][2] = {{1, 1}, {1, 0xFF}, {0xFF, 1}, {0xFF, 0xFF}, {0x53, 0x80}, {2, 0xFE}};
  for (size_t p = 0; p < t.ragged.mixed.patterns.size(); ++p) {
    const Pattern P = make_pattern(k, m, t, p);
    const int nT = static_cast<int>(P.T.size());
    CHECK(P.rows >= 4 && nT == k + P.rows);
    check_tables(k, t, t1, p, P, rng);
    uint8_t s[16];
    for (int j = 0; j < nT; ++j)
      for (uint8_t e : kValues) {
        syndromes(P, &j, &e, 1, s);
        CHECK(classify1_all(s, P.rows, P.k, P.gf, P.blk) == static_cast<uint32_t>(P.T[static_cast<size_t>(j)]));
        CHECK(classify2_all(s, P.rows, P.k, P.gf, P.blk) == static_cast<uint32_t>(P.T[static_cast<size_t>(j)]));
        ++g_wide_singles;
      }
    const int cand[] = {0, 1, 127, 128, k - 1, k, 254, 255};
    std::vector<int> at;
    for (int c : cand)
      if (c < nT && std::find(at.begin(), at.end(), c) == at.end()) at.push_back(c);
    const long before = g_pairs;
    for (size_t a = 0; a < at.size(); ++a)
      for (size_t b = a + 1; b < at.size(); ++b)
        for (const auto& e : kValuePairs) check_pair(P, at[a], at[b], e[0], e[1]);
    g_wide_pairs += g_pairs - before;
    check_seeded(P, rng);
  }
}

}  // namespace

int main() {
  for (int a = 0; a < 256; ++a)
    for (int b = 0; b < 256; ++b) g_mul[a][b] = gmul(static_cast<uint8_t>(a), static_cast<uint8_t>(b));
  std::mt19937 rng(20261020);
  {  // the z-table, exact for all 256 c: the even root of z^2 + z = c, or none
    LocateTables t;
    std::vector<uint8_t> pres(14, 1);
    const size_t size = 64;
    CHECK(build_locate_tables(10, 4, 1, &size, pres.data(), t, 2) == TableError::kOk);
    int with_root = 0;
    for (int c = 0; c < 256; ++c) {
      int roots = 0, even = -1;
      for (int z = 0; z < 256; ++z)
        if ((gmul(static_cast<uint8_t>(z), static_cast<uint8_t>(z)) ^ z) == c) {
          ++roots;
          if (!(z & 1)) even = z;
        }
      CHECK(roots == 0 || (roots == 2 && even >= 0));
      CHECK(t.gf[kLoc2Z + static_cast<size_t>(c)] == (roots ? even : 0xff));
      with_root += roots != 0;
    }
    CHECK(with_root == 128);
    // the multiply and divide the rule uses
    for (int a = 0; a < 256; ++a)
      for (int b = 0; b < 256; ++b) {
        CHECK(locate_mul(t.gf.data(), static_cast<uint32_t>(a), static_cast<uint32_t>(b)) == g_mul[a][b]);
        if (b) CHECK(locate_div(t.gf.data(), g_mul[a][b], static_cast<uint32_t>(b)) == static_cast<uint32_t>(a));
      }
    // RS(10,4), everything present: every pair of positions x every (e_a, e_b)
    const Pattern P = make_pattern(10, 4, t, 0);
    CHECK(P.rows == 4 && P.T.size() == 14);
    const long before = g_pairs;
    for (int a = 0; a < 14; ++a)
      for (int b = a + 1; b < 14; ++b)
        for (int ea = 1; ea < 256; ++ea)
          for (int eb = 1; eb < 256; ++eb) check_pair(P, a, b, static_cast<uint8_t>(ea), static_cast<uint8_t>(eb));
    CHECK(g_pairs - before == 91L * 255 * 255);
  }
  const int profiles[][2] = {{10, 4}, {1, 4}, {6, 4}, {16, 4}, {4, 5}, {10, 8}, {20, 12}, {10, 20}};
  for (const auto& pr : profiles) profile(pr[0], pr[1], false, rng);
  {  // RS(10,20), everything present, compares 16 rows
    LocateTables t;
    std::vector<uint8_t> pres(30, 1);
    const size_t size = 64;
    CHECK(build_locate_tables(10, 20, 1, &size, pres.data(), t, 2) == TableError::kOk);
    CHECK(t.rows(0) == 16);
  }
  // r' <= 3: the single rule's verdict
  const int shorts[][2] = {{10, 4}, {6, 3}, {4, 2}, {10, 8}};
  for (const auto& pr : shorts) profile(pr[0], pr[1], true, rng);
  CHECK(g_short > 0 && g_multis > 0);
  // positions, points and shard indices at and past 128; RS(240,16) with everything present
  // examines 256 shards, and position 255 has its own byte in the point table
  wide_profile(129, 9, {}, rng);
  wide_profile(240, 16, {1, 128}, rng);
  CHECK(g_wide_singles == 6L * (138 + 256 + 254));
  CHECK(g_wide_pairs == 6L * (10 + 28 + 15));  // 5, 8 and 6 distinct positions of the eight exist
  std::printf("wide singles %ld wide pairs %ld\n", g_wide_singles, g_wide_pairs);
  std::printf("singles %ld pairs %ld multis %ld short %ld\nlocate2_host_test ok\n", g_singles, g_pairs,
              g_multis, g_short);
  return 0;
}
