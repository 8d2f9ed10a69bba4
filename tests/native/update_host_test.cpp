// Host-side tables of update device plans and the overwrite planner on the
// CPU, built with g++ -fsanitize=address,undefined by tests/test_native_update.py:
//  - changed sets are deduplicated into patterns in order of first appearance, nsrc[p] counts
//    pattern p's changed shards and lists them in ascending order;
//  - every arena slice, evaluated byte by byte, is a scalar GF(2^8) multiply by P[j][i] for the
//    pattern's i-th changed shard and the launch group's row j (RS(10,20): 16 + 4 rows), and is
//    zero past the pattern's sources and past the group's rows; the pitch is cmax * 32 * W
//    rounded up to 256;
//  - the tile map holds only the stripes with a changed shard; a batch with none has no launch
//    group and no tile;
//  - the byte counts, and the refusals: a zero size on a changed stripe (not on an unchanged one);
//  - the overwrite planner against brute force over every (offset, len) of RS(4,2) at
//    S in {1, 5, 16}: at most three intervals, pairwise disjoint, covering exactly the touched
//    columns, each with exactly the shards changed at its columns.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "gf256.hpp"
#include "overwrite_plan.hpp"
#include "update_tables.hpp"

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

std::vector<uint8_t> flags_of(int k, const std::vector<std::vector<int>>& sets) {
  std::vector<uint8_t> f(sets.size() * static_cast<size_t>(k), 0);
  for (size_t b = 0; b < sets.size(); ++b)
    for (int i : sets[b]) f[b * k + i] = static_cast<uint8_t>(1 + (i % 3));  // any nonzero value is a flag
  return f;
}

void tables(int k, int m) {
  const std::vector<std::vector<int>> sets = {{0}, {k - 1}, {1, 2}, {}, {0}, {2, 1}, {k - 1}, {0, 1, 2}, {}};
  std::vector<std::vector<int>> norm = sets;
  for (auto& s : norm) std::sort(s.begin(), s.end());
  const std::vector<size_t> sizes = {17, 8192, 8193, 0, 5, 3 * 8192 + 1, 16, 40000, 123};
  const int batch = static_cast<int>(sets.size());
  const std::vector<uint8_t> fl = flags_of(k, sets);
  UpdateTables t;
  CHECK(build_update_tables(k, m, batch, sizes.data(), fl.data(), t) == TableError::kOk);
  // patterns in order of first appearance, deduplicated on the set (not on the flag values)
  const std::vector<std::vector<int>> want_patterns = {{0}, {k - 1}, {1, 2}, {0, 1, 2}};
  CHECK(t.patterns == want_patterns);
  CHECK(t.P() == 4 && t.cmax == 3);
  const std::vector<uint32_t> want_pat = {0, 1, 2, 0, 0, 2, 1, 3, 0};
  for (int b = 0; b < batch; ++b) {
    CHECK(t.has[b] == !sets[b].empty());
    if (t.has[b]) CHECK(t.pat[b] == want_pat[b] && t.patterns[t.pat[b]] == norm[b]);
    CHECK(t.size[b] == sizes[b]);
  }
  for (int p = 0; p < t.P(); ++p) CHECK(t.nsrc[p] == t.patterns[p].size());
  // the tile map: the changed stripes alone
  uint32_t ntiles = 0;
  std::vector<uint32_t> owners;
  for (int b = 0; b < batch; ++b) {
    if (sets[b].empty()) continue;
    CHECK(t.map.tile0[b] == ntiles);
    const uint32_t nt = static_cast<uint32_t>(ragged_tiles(sizes[b]));
    for (uint32_t q = 0; q < nt; ++q) owners.push_back(static_cast<uint32_t>(b));
    ntiles += nt;
  }
  CHECK(t.map.ntiles == ntiles && t.map.tile_stripe == owners && t.map.stripes == 7);
  CHECK(t.map.tile0[batch] == ntiles && t.map.any_tail);
  // bytes: sum over the changed stripes of size * (c * (2 | 1) + 2m)
  uint64_t bp = 0, bs = 0;
  for (int b = 0; b < batch; ++b)
    if (!sets[b].empty()) {
      bp += sizes[b] * (2 * sets[b].size() + 2 * static_cast<size_t>(m));
      bs += sizes[b] * (sets[b].size() + 2 * static_cast<size_t>(m));
    }
  CHECK(t.bytes_pair == bp && t.bytes_single == bs);
  // the arenas
  Mat E;
  CHECK(encode_matrix(k, m, E));
  CHECK(static_cast<int>(t.groups.size()) == (m + 15) / 16);
  int row0 = 0;
  for (const UpdateGroup& g : t.groups) {
    CHECK(g.row0 == row0 && g.R == std::min(16, m - row0));
    const size_t W = g.R > 8 ? 16 : 8;
    CHECK(g.tab_stride == (static_cast<size_t>(t.cmax) * 32 * W + 255) / 256 * 256);
    CHECK(g.tab_stride % 256 == 0 && g.arena.size() == g.tab_stride * t.patterns.size());
    for (int p = 0; p < t.P(); ++p) {
      const uint8_t* tab = &g.arena[p * g.tab_stride];
      for (size_t c = 0; c < static_cast<size_t>(t.cmax); ++c)
        for (int e = 0; e < 16; ++e)
          for (size_t r = 0; r < W; ++r) {
            const bool live = c < t.patterns[p].size() && static_cast<int>(r) < g.R;
            const uint8_t coef = live ? E.at(k + row0 + static_cast<int>(r), t.patterns[p][c]) : 0;
            if (live) CHECK(coef != 0);  // MDS: every entry of P is non-zero
            CHECK(tab[c * 32 * W + e * W + r] == slow_mul(coef, static_cast<uint8_t>(e)));
            CHECK(tab[c * 32 * W + (16 + e) * W + r] == slow_mul(coef, static_cast<uint8_t>(e << 4)));
          }
    }
    row0 += g.R;
  }
  CHECK(row0 == m);
  // a data byte through its two nibble lookups is the product
  const UpdateGroup& g0 = t.groups[0];
  const size_t W0 = g0.R > 8 ? 16 : 8;
  for (int x = 0; x < 256; ++x)
    CHECK((g0.arena[(x & 15) * W0] ^ g0.arena[(16 + (x >> 4)) * W0]) ==
          slow_mul(E.at(k, 0), static_cast<uint8_t>(x)));
}

void refusals_and_empty() {
  const int k = 4, m = 2;
  UpdateTables t;
  // nothing changed: no pattern, no group, no tile; sizes of 0 are fine
  const std::vector<size_t> sizes = {0, 100, 0};
  std::vector<uint8_t> none(3 * k, 0);
  CHECK(build_update_tables(k, m, 3, sizes.data(), none.data(), t) == TableError::kOk);
  CHECK(t.P() == 0 && t.cmax == 0 && t.groups.empty() && t.map.ntiles == 0 && t.map.stripes == 0);
  CHECK(t.bytes_pair == 0 && t.bytes_single == 0 && t.map.tile_stripe.empty());
  // a change in a stripe of size 0
  std::vector<uint8_t> one = none;
  one[2 * k + 1] = 1;
  CHECK(build_update_tables(k, m, 3, sizes.data(), one.data(), t) == TableError::kNoData);
  one[2 * k + 1] = 0;
  one[1 * k + 3] = 1;
  CHECK(build_update_tables(k, m, 3, sizes.data(), one.data(), t) == TableError::kOk);
  CHECK(t.P() == 1 && t.map.stripes == 1 && t.map.ntiles == 1 && t.map.tile_stripe[0] == 1);
  CHECK(t.bytes_pair == 100 * (2 + 4) && t.bytes_single == 100 * (1 + 4));
  // more tiles than a grid holds
  const std::vector<size_t> huge = {static_cast<size_t>(1) << 45};
  std::vector<uint8_t> f(k, 1);
  CHECK(build_update_tables(k, m, 1, huge.data(), f.data(), t) == TableError::kTooManyTiles);
}

void overwrite_brute_force() {
  const int k = 4;
  int plans = 0;
  for (size_t S : {static_cast<size_t>(1), static_cast<size_t>(5), static_cast<size_t>(16)}) {
    const uint64_t total = static_cast<uint64_t>(k) * S;
    std::vector<OverwriteInterval> iv;
    CHECK(!overwrite_plan(k, S, 0, 0, iv) && iv.empty());
    CHECK(!overwrite_plan(k, S, total, 1, iv));
    CHECK(!overwrite_plan(k, S, 0, total + 1, iv));
    CHECK(!overwrite_plan(k, S, total - 1, 2, iv));
    CHECK(!overwrite_plan(k, S, 1, ~static_cast<uint64_t>(0), iv));
    CHECK(!overwrite_plan(k, 0, 0, 1, iv));
    for (uint64_t off = 0; off < total; ++off)
      for (uint64_t len = 1; off + len <= total; ++len) {
        CHECK(overwrite_plan(k, S, off, len, iv));
        ++plans;
        CHECK(!iv.empty() && iv.size() <= 3);
        // what changes at each column
        std::vector<std::set<int>> truth(S);
        for (uint64_t x = off; x < off + len; ++x) truth[x % S].insert(static_cast<int>(x / S));
        std::vector<int> covered(S, 0);
        size_t prev_end = 0;
        for (const OverwriteInterval& q : iv) {
          CHECK(q.col0 < q.col1 && q.col1 <= S && q.col0 >= prev_end);  // ascending, disjoint
          CHECK(0 <= q.shard0 && q.shard0 <= q.shard1 && q.shard1 < k);
          prev_end = q.col1;
          std::set<int> set;
          for (int i = q.shard0; i <= q.shard1; ++i) set.insert(i);
          for (size_t c = q.col0; c < q.col1; ++c) {
            ++covered[c];
            CHECK(truth[c] == set);
          }
        }
        for (size_t c = 0; c < S; ++c) CHECK(covered[c] == (truth[c].empty() ? 0 : 1));
      }
  }
  CHECK(plans == 4 * 5 / 2 + 20 * 21 / 2 + 64 * 65 / 2);
}

}  // namespace

int main() {
  tables(10, 4);
  tables(10, 20);
  tables(3, 9);
  refusals_and_empty();
  overwrite_brute_force();
  std::printf("update_host_test ok\n");
  return 0;
}
