// Host-side tables of decode-idx device plans on the CPU, built with
// g++ -fsanitize=address,undefined by tests/test_native_decode_idx.py:
//  - (expected, wanted, delivered) triples are deduplicated into patterns in order of first
//    appearance over the stripes with both a delivered and a wanted shard; nsrc[p] and nrows[p]
//    count the pattern's delivered and wanted shards, listed ascending; one inversion per
//    expected set;
//  - every C entry equals the entry of decode_plan's row (what rs_decode_rows returns) for a
//    presence mask equal to the expected set, and is nonzero (E is MDS: a zero entry would make
//    k rows of E dependent), over seeded expected sets that include parity shards;
//  - every arena slice, evaluated byte by byte, is a bit-by-bit GF(2^8) multiply by C[w][v] for
//    the pattern's delivered shard and the launch group's row, and zero past the pattern's
//    sources and rows; the pitch is cmax * 32 * W rounded up to 256; more than 16 wanted rows
//    make a second launch group;
//  - the tile map holds only the stripes with both; a batch with none has no group and no tile;
//  - the byte counts, and every refusal in the stated order.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "decode_idx_tables.hpp"
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
  std::vector<int> expect, wanted, delivered;
  size_t size;
};

struct Flags {
  std::vector<uint8_t> expect, in, dst;
  std::vector<size_t> sizes;
};

Flags flags_of(int n, const std::vector<Stripe>& st) {
  Flags f;
  f.expect.assign(st.size() * n, 0);
  f.in = f.dst = f.expect;
  for (size_t b = 0; b < st.size(); ++b) {
    for (int i : st[b].expect) f.expect[b * n + i] = static_cast<uint8_t>(1 + (i % 3));  // any nonzero value
    for (int i : st[b].delivered) f.in[b * n + i] = 1;
    for (int i : st[b].wanted) f.dst[b * n + i] = 7;
    f.sizes.push_back(st[b].size);
  }
  return f;
}

std::vector<int> sorted(std::vector<int> v) {
  std::sort(v.begin(), v.end());
  return v;
}

// k of the n indices, seeded; `parity` of them forced to be parity shards where the profile allows
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

void check_tables(int k, int m, const std::vector<Stripe>& st, const DecodeIdxTables& t) {
  const int n = k + m;
  const int batch = static_cast<int>(st.size());
  // patterns: first appearance over the stripes in the launch
  std::vector<std::vector<std::vector<int>>> firsts;
  uint32_t ntiles = 0;
  std::vector<uint32_t> owners;
  uint64_t bm = 0, bs = 0;
  int stripes = 0, cmax = 0, rmax = 0;
  bool tail = false;
  std::set<std::vector<int>> esets;
  for (int b = 0; b < batch; ++b) {
    const bool has = !st[b].delivered.empty() && !st[b].wanted.empty();
    CHECK(t.has[b] == has && t.size[b] == st[b].size);
    if (!has) continue;
    const std::vector<std::vector<int>> tri = {sorted(st[b].expect), sorted(st[b].wanted), sorted(st[b].delivered)};
    size_t p = 0;
    while (p < firsts.size() && firsts[p] != tri) ++p;
    if (p == firsts.size()) firsts.push_back(tri);
    CHECK(t.pat[b] == p);
    esets.insert(tri[0]);
    CHECK(t.map.tile0[b] == ntiles);
    const uint32_t nt = static_cast<uint32_t>(ragged_tiles(st[b].size));
    for (uint32_t q = 0; q < nt; ++q) owners.push_back(static_cast<uint32_t>(b));
    ntiles += nt;
    ++stripes;
    tail |= st[b].size % 16 != 0;
    bm += st[b].size * (tri[2].size() + 2 * tri[1].size());
    bs += st[b].size * (tri[2].size() + tri[1].size());
    cmax = std::max(cmax, static_cast<int>(tri[2].size()));
    rmax = std::max(rmax, static_cast<int>(tri[1].size()));
  }
  CHECK(t.map.ntiles == ntiles && t.map.tile_stripe == owners && t.map.stripes == stripes);
  CHECK(t.map.tile0[batch] == ntiles && t.map.any_tail == tail);
  CHECK(t.bytes_merge == bm && t.bytes_store == bs);
  CHECK(t.P() == static_cast<int>(firsts.size()) && t.cmax == cmax && t.rmax == rmax);
  CHECK(t.inversions == static_cast<int>(esets.size()));
  CHECK(static_cast<int>(t.groups.size()) == (rmax + 15) / 16);
  for (int p = 0; p < t.P(); ++p) {
    const DecodeIdxPattern& pt = t.patterns[p];
    CHECK(pt.expect == firsts[p][0] && pt.wanted == firsts[p][1] && pt.delivered == firsts[p][2]);
    CHECK(t.nsrc[p] == pt.delivered.size() && t.nrows[p] == pt.wanted.size());
    CHECK(static_cast<int>(pt.expect.size()) == k);
    // the rows a reconstruct with exactly the expected shards present uses
    std::vector<uint8_t> present(n, 0);
    for (int i : pt.expect) present[i] = 1;
    DecodePlan dp;
    CHECK(decode_plan(k, m, present.data(), dp));
    CHECK(dp.valid == pt.expect && dp.check.empty() && static_cast<int>(dp.missing.size()) == m);
    for (size_t r = 0; r < pt.wanted.size(); ++r) {
      const int row = static_cast<int>(std::find(dp.missing.begin(), dp.missing.end(), pt.wanted[r]) - dp.missing.begin());
      CHECK(row < m);
      for (size_t c = 0; c < pt.delivered.size(); ++c) {
        CHECK(pt.expect[pt.col[c]] == pt.delivered[c]);
        const uint8_t want = dp.rows.at(row, pt.col[c]);
        CHECK(pt.C.at(static_cast<int>(r), static_cast<int>(c)) == want);
        CHECK(want != 0);
      }
      // (and every other entry of the row: the MDS condition over the whole expected set)
      for (int c = 0; c < k; ++c) CHECK(dp.rows.at(row, c) != 0);
    }
  }
  // the arenas, byte by byte
  int row0 = 0;
  for (const DecodeIdxGroup& g : t.groups) {
    CHECK(g.row0 == row0 && g.R == std::min(16, rmax - row0));
    const int W = nibble_width(g.R);
    CHECK(W == (g.R > 8 ? 16 : 8));
    const size_t per = 32u * static_cast<size_t>(W);
    CHECK(g.tab_stride == (static_cast<size_t>(cmax) * per + 255) / 256 * 256);
    CHECK(g.arena.size() == t.patterns.size() * g.tab_stride && g.nrows.size() == t.patterns.size());
    for (int p = 0; p < t.P(); ++p) {
      const DecodeIdxPattern& pt = t.patterns[p];
      const int have = std::max(0, std::min(g.R, static_cast<int>(pt.wanted.size()) - row0));
      CHECK(g.nrows[p] == static_cast<uint32_t>(have));
      const uint8_t* base = &g.arena[p * g.tab_stride];
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
  const int k = 10, m = 4, n = 14;
  const std::vector<int> first = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, last = {4, 5, 6, 7, 8, 9, 10, 11, 12, 13};
  const std::vector<int> mix = {0, 2, 3, 5, 6, 8, 9, 10, 12, 13};
  const std::vector<Stripe> st = {
      {first, {10, 11, 12, 13}, {0}, 17},           // pattern 0
      {last, {0, 1, 2, 3}, {13, 4}, 8192},          // pattern 1
      {first, {10, 11, 12, 13}, {}, 99},            // nothing delivered: in no launch
      {mix, {1, 11}, {0, 2, 12}, 8193},             // pattern 2
      {first, {13, 12, 11, 10}, {0}, 5},            // pattern 0 again (order of the lists is not the key)
      {mix, {}, {0, 2, 12}, 0},                     // nothing wanted: in no launch, size 0 is fine
      {last, {0, 1, 2, 3}, {4, 13}, 3 * 8192 + 1},  // pattern 1 again
      {first, {10}, {0}, 16},                       // pattern 3: same sets but one wanted
      {first, {10, 11, 12, 13}, {1}, 40000},        // pattern 4: another delivered shard
  };
  const Flags f = flags_of(n, st);
  DecodeIdxTables t;
  CHECK(build_decode_idx_tables(k, m, static_cast<int>(st.size()), f.sizes.data(), f.expect.data(), f.in.data(),
                                f.dst.data(), t) == DecodeIdxError::kOk);
  const std::vector<uint32_t> want_pat = {0, 1, 0, 2, 0, 0, 1, 3, 4};
  for (size_t b = 0; b < st.size(); ++b)
    if (t.has[b]) CHECK(t.pat[b] == want_pat[b]);
  CHECK(t.P() == 5 && t.cmax == 3 && t.rmax == 4 && t.inversions == 3 && t.map.stripes == 7);
  const std::vector<uint32_t> nsrc = {1, 2, 3, 1, 1}, nrows = {4, 4, 2, 1, 4};
  CHECK(t.nsrc == nsrc && t.nrows == nrows);
  CHECK(t.groups.size() == 1 && t.groups[0].R == 4 && t.groups[0].nrows == nrows);
  check_tables(k, m, st, t);

  // nothing delivered anywhere: no group, no tile, no pattern
  std::vector<Stripe> idle = {st[2], st[5]};
  const Flags fi = flags_of(n, idle);
  CHECK(build_decode_idx_tables(k, m, 2, fi.sizes.data(), fi.expect.data(), fi.in.data(), fi.dst.data(), t) ==
        DecodeIdxError::kOk);
  CHECK(t.groups.empty() && t.map.ntiles == 0 && t.P() == 0 && t.cmax == 0 && t.bytes_merge == 0);
}

void refusals() {
  const int k = 4, m = 2, n = 6;
  auto build = [&](const std::vector<Stripe>& st) {
    const Flags f = flags_of(n, st);
    DecodeIdxTables t;
    return build_decode_idx_tables(k, m, static_cast<int>(st.size()), f.sizes.data(), f.expect.data(), f.in.data(),
                                   f.dst.data(), t);
  };
  const Stripe good = {{0, 1, 2, 3}, {4, 5}, {0}, 16};
  CHECK(build({good}) == DecodeIdxError::kOk);
  const Stripe few = {{0, 1, 2}, {4}, {0}, 16}, many = {{0, 1, 2, 3, 4}, {5}, {0}, 16};
  const Stripe in_unexpected = {{0, 1, 2, 3}, {5}, {4}, 16}, dst_expected = {{0, 1, 2, 3}, {3}, {0}, 16};
  const Stripe zero = {{0, 1, 2, 3}, {4}, {0}, 0};
  const Stripe zero_idle_in = {{0, 1, 2, 3}, {4}, {}, 0}, zero_idle_dst = {{0, 1, 2, 3}, {}, {1}, 0};
  CHECK(build({few}) == DecodeIdxError::kTooFewShards);
  CHECK(build({many}) == DecodeIdxError::kArg);
  CHECK(build({in_unexpected}) == DecodeIdxError::kArg);
  CHECK(build({dst_expected}) == DecodeIdxError::kArg);
  CHECK(build({zero}) == DecodeIdxError::kNoData);
  // a zero size on a stripe that is in no launch is no error
  CHECK(build({zero_idle_in, zero_idle_dst, good}) == DecodeIdxError::kOk);
  // the order: the expected counts of the whole batch, then the misplaced pointers, then sizes
  CHECK(build({zero, in_unexpected, few}) == DecodeIdxError::kTooFewShards);
  CHECK(build({zero, dst_expected, many}) == DecodeIdxError::kArg);
  CHECK(build({many, few}) == DecodeIdxError::kArg);  // within a check, the first stripe
  CHECK(build({few, many}) == DecodeIdxError::kTooFewShards);
  CHECK(build({zero, in_unexpected}) == DecodeIdxError::kArg);
  CHECK(build({zero, dst_expected}) == DecodeIdxError::kArg);
  // a misplaced pointer on a stripe with a short expected set reports the set
  const Stripe few_and_misplaced = {{0, 1, 2}, {0}, {5}, 0};
  CHECK(build({few_and_misplaced}) == DecodeIdxError::kTooFewShards);
}

// Seeded expected sets with parity shards, wanted and delivered subsets, every entry checked.
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
    // all of them first (more than 16 rows where m > 16), then subsets
    const size_t nw = b < 2 ? rest.size() : 1 + rng() % rest.size();
    s.wanted.assign(rest.begin(), rest.begin() + static_cast<ptrdiff_t>(nw));
    std::vector<int> e = s.expect;
    std::shuffle(e.begin(), e.end(), rng);
    const size_t nd = b == 1 ? e.size() : 1 + rng() % e.size();
    s.delivered.assign(e.begin(), e.begin() + static_cast<ptrdiff_t>(nd));
    s.size = sizes[b];
    st.push_back(s);
  }
  const Flags f = flags_of(n, st);
  DecodeIdxTables t;
  CHECK(build_decode_idx_tables(k, m, static_cast<int>(st.size()), f.sizes.data(), f.expect.data(), f.in.data(),
                                f.dst.data(), t) == DecodeIdxError::kOk);
  CHECK(t.cmax == k && t.rmax == m);
  CHECK(static_cast<int>(t.groups.size()) == (m + 15) / 16);
  check_tables(k, m, st, t);
}

}  // namespace

int main() {
  dedup_and_map();
  refusals();
  const int profiles[][2] = {{10, 4}, {4, 2}, {3, 2}, {1, 3}, {16, 4}, {10, 8}, {20, 12}, {10, 20}};
  uint32_t seed = 2024;
  for (const auto& p : profiles) profile(p[0], p[1], seed++);
  std::printf("decode_idx_host_test ok\n");
  return 0;
}
