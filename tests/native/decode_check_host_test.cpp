// Host-side tables of decode-check device plans on the CPU, built with
// g++ -fsanitize=address,undefined by tests/test_native_decode_check.py:
//  - (expected, wanted, compared, delivered) patterns are deduplicated in order of first
//    appearance over the stripes in the launch; a final build also takes a stripe with a check row
//    and nothing delivered; the row list is wanted and compared ascending, the source list is
//    delivered ascending, expected and compared sources alike; one inversion per expected set;
//  - an expected source's column is decode_plan's row entry (nonzero: E is MDS), a compared
//    source's column is the unit column of its own check row;
//  - cmask per launch group, with a check row on each side of the 16-row boundary of RS(10,20);
//  - every arena byte against a bit-by-bit GF(2^8) multiply;
//  - the byte counts in all four flag combinations, the tile map, every refusal in its order.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "decode_check_tables.hpp"
#include "gf256.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// bit-by-bit multiply mod 0x11D: independent of gf256.hpp's log / exp tables
uint8_t slow_mul(uint8_t a, uint8_t b) {
  unsigned r = 0, x = a;
  for (int bit = 0; bit < 8; ++bit) {
    if ((b >> bit) & 1u) r ^= x;
    x <<= 1;
    if (x & 0x100u) x ^= 0x11Du;
  }
  return static_cast<uint8_t>(r);
}

struct Stripe {
  std::vector<int> expect, wanted, compared, delivered;
  size_t size;
};

struct Flags {
  std::vector<uint8_t> expect, in, dst, chk;
  std::vector<size_t> sizes;
};

Flags flags_of(int n, const std::vector<Stripe>& st) {
  Flags f;
  f.expect.assign(st.size() * n, 0);
  f.in = f.dst = f.chk = f.expect;
  for (size_t b = 0; b < st.size(); ++b) {
    for (int i : st[b].expect) f.expect[b * n + i] = static_cast<uint8_t>(1 + (i % 3));  // any nonzero value
    for (int i : st[b].delivered) f.in[b * n + i] = 1;
    for (int i : st[b].wanted) f.dst[b * n + i] = 7;
    for (int i : st[b].compared) f.chk[b * n + i] = 9;
    f.sizes.push_back(st[b].size);
  }
  return f;
}

std::vector<int> sorted(std::vector<int> v) {
  std::sort(v.begin(), v.end());
  return v;
}

DecodeIdxError build(int k, int m, const std::vector<Stripe>& st, bool final, DecodeCheckTables& t) {
  const Flags f = flags_of(k + m, st);
  return build_decode_check_tables(k, m, static_cast<int>(st.size()), f.sizes.data(), f.expect.data(), f.in.data(),
                                   f.dst.data(), f.chk.data(), final, t);
}

bool in_launch(const Stripe& s, bool final) {
  const bool row = !s.wanted.empty() || !s.compared.empty();
  return (!s.delivered.empty() && row) || (final && !s.compared.empty());
}

void check_tables(int k, int m, const std::vector<Stripe>& st, bool final, const DecodeCheckTables& t) {
  const int n = k + m;
  const int batch = static_cast<int>(st.size());
  std::vector<std::vector<std::vector<int>>> firsts;
  uint32_t ntiles = 0;
  std::vector<uint32_t> owners;
  uint64_t bytes[4] = {0, 0, 0, 0};
  int stripes = 0, cmax = 0, rmax = 0;
  bool tail = false;
  std::set<std::vector<int>> esets;
  for (int b = 0; b < batch; ++b) {
    const bool has = in_launch(st[b], final);
    CHECK(t.has[b] == has && t.size[b] == st[b].size);
    if (!has) continue;
    const std::vector<std::vector<int>> quad = {sorted(st[b].expect), sorted(st[b].wanted), sorted(st[b].compared),
                                                sorted(st[b].delivered)};
    size_t p = 0;
    while (p < firsts.size() && firsts[p] != quad) ++p;
    if (p == firsts.size()) firsts.push_back(quad);
    CHECK(t.pat[b] == p);
    esets.insert(quad[0]);
    CHECK(t.map.tile0[b] == ntiles);
    const uint32_t nt = static_cast<uint32_t>(ragged_tiles(st[b].size));
    for (uint32_t q = 0; q < nt; ++q) owners.push_back(static_cast<uint32_t>(b));
    ntiles += nt;
    ++stripes;
    tail |= st[b].size % 16 != 0;
    const uint64_t S = st[b].size, c = quad[3].size(), w = quad[1].size(), x = quad[2].size();
    bytes[0] += S * (c + 2 * w + 2 * x);  // merge
    bytes[1] += S * (c + w + x);          // store
    bytes[2] += S * (c + 2 * w + x);      // final merge
    bytes[3] += S * (c + w);              // final store
    cmax = std::max(cmax, static_cast<int>(c));
    rmax = std::max(rmax, static_cast<int>(w + x));
  }
  CHECK(t.map.ntiles == ntiles && t.map.tile_stripe == owners && t.map.stripes == stripes);
  CHECK(t.map.tile0[batch] == ntiles && t.map.any_tail == tail);
  for (int i = 0; i < 4; ++i) CHECK(t.bytes[i] == bytes[i]);
  CHECK(t.P() == static_cast<int>(firsts.size()) && t.cmax == cmax && t.rmax == rmax);
  CHECK(t.inversions == static_cast<int>(esets.size()));
  CHECK(static_cast<int>(t.groups.size()) == (rmax + 15) / 16);
  for (int p = 0; p < t.P(); ++p) {
    const DecodeCheckPattern& pt = t.patterns[p];
    std::vector<int> rows = firsts[p][1];
    rows.insert(rows.end(), firsts[p][2].begin(), firsts[p][2].end());
    rows = sorted(rows);
    CHECK(pt.expect == firsts[p][0] && pt.rows == rows && pt.delivered == firsts[p][3]);
    CHECK(pt.check.size() == rows.size() && pt.col.size() == pt.delivered.size());
    for (size_t r = 0; r < rows.size(); ++r)
      CHECK((pt.check[r] != 0) == (std::count(firsts[p][2].begin(), firsts[p][2].end(), rows[r]) != 0));
    CHECK(t.nsrc[p] == pt.delivered.size() && t.nrows[p] == rows.size());
    CHECK(static_cast<int>(pt.expect.size()) == k);
    std::vector<uint8_t> present(n, 0);
    for (int i : pt.expect) present[i] = 1;
    DecodePlan dp;
    CHECK(decode_plan(k, m, present.data(), dp));
    CHECK(dp.valid == pt.expect && static_cast<int>(dp.missing.size()) == m);
    for (size_t r = 0; r < rows.size(); ++r) {
      const int row = static_cast<int>(std::find(dp.missing.begin(), dp.missing.end(), rows[r]) - dp.missing.begin());
      CHECK(row < m);
      for (size_t c = 0; c < pt.delivered.size(); ++c) {
        const uint8_t got = pt.C.at(static_cast<int>(r), static_cast<int>(c));
        if (pt.col[c] >= 0) {
          CHECK(pt.expect[pt.col[c]] == pt.delivered[c]);
          CHECK(got == dp.rows.at(row, pt.col[c]) && got != 0);
        } else {
          // a compared source: the unit column of its own check row
          CHECK(!present[pt.delivered[c]]);
          CHECK(std::count(firsts[p][2].begin(), firsts[p][2].end(), pt.delivered[c]) == 1);
          CHECK(got == (pt.delivered[c] == rows[r] ? 1 : 0));
        }
      }
      for (int c = 0; c < k; ++c) CHECK(dp.rows.at(row, c) != 0);  // an expected error reaches every row
    }
  }
  int row0 = 0;
  for (const DecodeCheckGroup& g : t.groups) {
    CHECK(g.row0 == row0 && g.R == std::min(16, rmax - row0));
    const int W = nibble_width(g.R);
    CHECK(W == (g.R > 8 ? 16 : 8));
    const size_t per = 32u * static_cast<size_t>(W);
    CHECK(g.tab_stride == (static_cast<size_t>(cmax) * per + 255) / 256 * 256);
    CHECK(g.arena.size() == t.patterns.size() * g.tab_stride && g.nrows.size() == t.patterns.size());
    CHECK(g.cmask.size() == t.patterns.size());
    for (int p = 0; p < t.P(); ++p) {
      const DecodeCheckPattern& pt = t.patterns[p];
      const int have = std::max(0, std::min(g.R, static_cast<int>(pt.rows.size()) - row0));
      CHECK(g.nrows[p] == static_cast<uint32_t>(have));
      uint32_t cm = 0;
      for (int r = 0; r < have; ++r)
        if (pt.check[static_cast<size_t>(row0 + r)]) cm |= 1u << r;
      CHECK(g.cmask[p] == cm);
      const uint8_t* base = g.arena.data() + p * g.tab_stride;
      for (size_t off = 0; off < g.tab_stride; ++off) {
        const size_t c = off / per, e = (off % per) / W, r = off % W;
        uint8_t want = 0;
        if (have > 0 && c < pt.delivered.size() && static_cast<int>(r) < have) {
          const uint8_t coef = pt.C.at(row0 + static_cast<int>(r), static_cast<int>(c));
          want = slow_mul(coef, static_cast<uint8_t>(e < 16 ? e : (e - 16) << 4));
        }
        CHECK(base[off] == want);
      }
    }
    row0 += g.R;
  }
}

void dedup_and_map() {
  const int k = 10, m = 4;
  const std::vector<int> first = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, last = {4, 5, 6, 7, 8, 9, 10, 11, 12, 13};
  const std::vector<int> mix = {0, 2, 3, 5, 6, 8, 9, 10, 12, 13};
  const std::vector<Stripe> st = {
      {first, {10, 11}, {12, 13}, {0}, 17},            // pattern 0
      {last, {0, 1}, {3}, {13, 4, 3}, 8192},           // pattern 1: the compared shard arrives too
      {first, {10, 11}, {12, 13}, {}, 99},             // nothing delivered: a final launch only (pattern 2 there)
      {mix, {1}, {11}, {0, 2, 12}, 8193},              // next pattern
      {first, {11, 10}, {13, 12}, {0}, 5},             // pattern 0 again (order of the lists is not the key)
      {mix, {}, {}, {0, 2, 12}, 0},                    // no row: in no launch, size 0 is fine
      {first, {10, 11, 12}, {13}, {0}, 16},            // same indices as pattern 0, another split
      {first, {}, {12, 13}, {12}, 40000},              // compared alone, one of them delivered
      {first, {10, 11}, {}, {}, 0},                    // wanted alone, nothing delivered: in no launch
  };
  for (const bool final : {false, true}) {
    DecodeCheckTables t;
    CHECK(build(k, m, st, final, t) == DecodeIdxError::kOk);
    const std::vector<uint32_t> pat = final ? std::vector<uint32_t>{0, 1, 2, 3, 0, 0, 4, 5, 0}
                                            : std::vector<uint32_t>{0, 1, 0, 2, 0, 0, 3, 4, 0};
    for (size_t b = 0; b < st.size(); ++b)
      if (t.has[b]) CHECK(t.pat[b] == pat[b]);
    CHECK(t.has[2] == (final ? 1 : 0) && !t.has[5] && !t.has[8]);
    CHECK(t.P() == (final ? 6 : 5) && t.cmax == 3 && t.rmax == 4 && t.inversions == 3);
    const std::vector<uint32_t> nsrc = final ? std::vector<uint32_t>{1, 3, 0, 3, 1, 1} : std::vector<uint32_t>{1, 3, 3, 1, 1};
    const std::vector<uint32_t> cmask = final ? std::vector<uint32_t>{12, 4, 12, 2, 8, 3}
                                              : std::vector<uint32_t>{12, 4, 2, 8, 3};
    CHECK(t.nsrc == nsrc && t.groups.size() == 1 && t.groups[0].cmask == cmask);
    check_tables(k, m, st, final, t);
  }
  // pattern 1's unit column: shard 3 is source 0 (3 < 4 < 13) and row 2 (0, 1, 3)
  {
    DecodeCheckTables t;
    CHECK(build(k, m, st, false, t) == DecodeIdxError::kOk);
    const DecodeCheckPattern& p = t.patterns[1];
    CHECK(p.delivered == (std::vector<int>{3, 4, 13}) && p.rows == (std::vector<int>{0, 1, 3}));
    CHECK(p.col[0] == -1 && p.C.at(0, 0) == 0 && p.C.at(1, 0) == 0 && p.C.at(2, 0) == 1);
  }
  // a final batch with nothing delivered anywhere: cmax 0, empty arenas, the stripes mapped
  {
    const std::vector<Stripe> idle = {st[2], st[8], {last, {}, {0}, {}, 8193}};
    DecodeCheckTables t;
    CHECK(build(k, m, idle, true, t) == DecodeIdxError::kOk);
    CHECK(t.cmax == 0 && t.P() == 2 && t.has[0] && !t.has[1] && t.has[2] && t.map.stripes == 2);
    CHECK(t.map.ntiles == ragged_tiles(99) + ragged_tiles(8193));
    CHECK(t.groups.size() == 1 && t.groups[0].tab_stride == 0 && t.groups[0].arena.empty());
    CHECK(t.groups[0].nrows == (std::vector<uint32_t>{4, 1}) && t.groups[0].cmask == (std::vector<uint32_t>{12, 1}));
    CHECK(t.bytes[2] == 99u * 6 + 8193u && t.bytes[3] == 99u * 2);
    check_tables(k, m, idle, true, t);
    // the same batch without FINAL: nothing to launch
    CHECK(build(k, m, idle, false, t) == DecodeIdxError::kOk);
    CHECK(t.groups.empty() && t.map.ntiles == 0 && t.P() == 0 && t.bytes[0] == 0);
  }
}

// RS(10,20): 20 rows in two launch groups, with check rows 15 and 16 on either side of the boundary
void two_groups() {
  const int k = 10, m = 20;
  std::vector<int> expect, wanted, compared;
  for (int i = 0; i < 10; ++i) expect.push_back(i);
  for (int i = 10; i < 30; ++i) (i == 25 || i == 26 || i == 29 ? compared : wanted).push_back(i);
  const std::vector<Stripe> st = {{expect, wanted, compared, {3, 25, 26}, 8193}};
  DecodeCheckTables t;
  CHECK(build(k, m, st, true, t) == DecodeIdxError::kOk);
  CHECK(t.groups.size() == 2 && t.groups[0].R == 16 && t.groups[1].R == 4);
  CHECK(t.groups[0].cmask[0] == 1u << 15 && t.groups[1].cmask[0] == (1u | 8u));
  check_tables(k, m, st, true, t);
}

void refusals() {
  const int k = 4, m = 2;
  for (const bool final : {false, true}) {
    auto go = [&](const std::vector<Stripe>& st) {
      DecodeCheckTables t;
      return build(k, m, st, final, t);
    };
    const Stripe good = {{0, 1, 2, 3}, {4}, {5}, {0, 5}, 16};
    CHECK(go({good}) == DecodeIdxError::kOk);
    const Stripe few = {{0, 1, 2}, {4}, {}, {0}, 16}, many = {{0, 1, 2, 3, 4}, {5}, {}, {0}, 16};
    const Stripe in_unexpected = {{0, 1, 2, 3}, {5}, {}, {4}, 16}, in_wanted = {{0, 1, 2, 3}, {4}, {5}, {4}, 16};
    const Stripe dst_expected = {{0, 1, 2, 3}, {3}, {}, {0}, 16}, chk_expected = {{0, 1, 2, 3}, {}, {3}, {0}, 16};
    const Stripe chk_and_dst = {{0, 1, 2, 3}, {4}, {4}, {0}, 16};
    const Stripe zero = {{0, 1, 2, 3}, {}, {4}, {0}, 0};
    const Stripe zero_scan = {{0, 1, 2, 3}, {}, {4}, {}, 0};  // in a final launch alone
    const Stripe zero_idle = {{0, 1, 2, 3}, {4}, {}, {}, 0};
    CHECK(go({few}) == DecodeIdxError::kTooFewShards);
    CHECK(go({many}) == DecodeIdxError::kArg);
    for (const Stripe& s : {in_unexpected, in_wanted, dst_expected, chk_expected, chk_and_dst}) {
      CHECK(go({s}) == DecodeIdxError::kArg);
      CHECK(go({zero, s}) == DecodeIdxError::kArg);                // before the sizes
      CHECK(go({zero, s, few}) == DecodeIdxError::kTooFewShards);  // after the expected counts
    }
    CHECK(go({zero}) == DecodeIdxError::kNoData);
    CHECK(go({zero_scan}) == (final ? DecodeIdxError::kNoData : DecodeIdxError::kOk));
    CHECK(go({zero_idle, good}) == DecodeIdxError::kOk);
    CHECK(go({many, few}) == DecodeIdxError::kArg);  // within a check, the first stripe
    CHECK(go({few, many}) == DecodeIdxError::kTooFewShards);
  }
}

// k of the n indices, seeded, `parity` of them parity shards where the profile allows
std::vector<int> expected_set(std::mt19937& rng, int k, int m, int parity) {
  std::vector<int> data(k), par(m);
  for (int i = 0; i < k; ++i) data[i] = i;
  for (int j = 0; j < m; ++j) par[j] = k + j;
  std::shuffle(data.begin(), data.end(), rng);
  std::shuffle(par.begin(), par.end(), rng);
  parity = std::min(parity, std::min(k, m));
  std::vector<int> e(par.begin(), par.begin() + parity);
  e.insert(e.end(), data.begin(), data.begin() + (k - parity));
  return sorted(e);
}

// Seeded expected sets with parity shards; the rest split into wanted, compared and unused;
// expected and compared shards delivered in seeded subsets; every entry checked.
void profile(int k, int m, uint32_t seed) {
  std::mt19937 rng(seed);
  const int n = k + m;
  std::vector<Stripe> st;
  const size_t sizes[] = {1, 17, 8192, 8193, 16};
  for (int b = 0; b < 5; ++b) {
    Stripe s;
    s.expect = expected_set(rng, k, m, b == 0 ? 0 : 1 + static_cast<int>(rng() % static_cast<unsigned>(m)));
    std::vector<uint8_t> isexp(n, 0);
    for (int i : s.expect) isexp[i] = 1;
    std::vector<int> rest;
    for (int i = 0; i < n; ++i)
      if (!isexp[i]) rest.push_back(i);
    std::shuffle(rest.begin(), rest.end(), rng);
    // every other index in a row first (more than 16 rows where m > 16), then subsets
    const size_t nr = b < 2 ? rest.size() : 1 + rng() % rest.size();
    for (size_t i = 0; i < nr; ++i) (rng() % 2 || (b == 0 && i == 0) ? s.compared : s.wanted).push_back(rest[i]);
    std::vector<int> e = s.expect;
    std::shuffle(e.begin(), e.end(), rng);
    const size_t nd = b == 1 ? e.size() : b == 4 ? 0 : 1 + rng() % e.size();
    s.delivered.assign(e.begin(), e.begin() + static_cast<ptrdiff_t>(nd));
    for (int j : s.compared)
      if (rng() % 2) s.delivered.push_back(j);
    s.size = sizes[b];
    st.push_back(s);
  }
  for (const bool final : {false, true}) {
    DecodeCheckTables t;
    CHECK(build(k, m, st, final, t) == DecodeIdxError::kOk);
    CHECK(t.rmax == m);
    check_tables(k, m, st, final, t);
  }
}

}  // namespace

int main() {
  dedup_and_map();
  two_groups();
  refusals();
  const int profiles[][2] = {{10, 4}, {4, 2}, {3, 2}, {1, 3}, {16, 4}, {10, 8}, {20, 12}, {10, 20}};
  uint32_t seed = 2025;
  for (const auto& p : profiles) profile(p[0], p[1], seed++);
  std::printf("decode_check_host_test ok\n");
  return 0;
}
