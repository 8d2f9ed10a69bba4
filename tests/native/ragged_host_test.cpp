// Host-side tables of ragged device plans (callfs_amd/csrc/ragged_tables.hpp) on the CPU,
// built with g++ -fsanitize=address,undefined by tests/test_native_ragged.py.
// The tile map of batches of different shard sizes: tile0 (the prefix sums), tile_stripe
// entry by entry and ntiles, for sizes on both sides of the vector and the tile edges; a
// zero size and a tile total past the grid limit are reported; and the pattern, arena and
// compare-mask pieces equal build_mixed_tables' for the same masks.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gf256.hpp"
#include "mixed_tables.hpp"
#include "ragged_tables.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// tiles of one stripe, from the definition: 8,192-byte tiles over the whole vectors, one
// tile for a stripe that has less than a tile of them (or none)
uint32_t want_tiles(size_t S) {
  const size_t whole = S / 16 * 16;
  uint32_t t = 0;
  for (size_t at = 0; at < whole; at += 8192) ++t;
  return t ? t : 1;
}

void check_map(const std::vector<size_t>& sizes) {
  const int batch = static_cast<int>(sizes.size());
  TileMap t;
  CHECK(build_tile_map(batch, sizes.data(), nullptr, t) == TableError::kOk);
  CHECK(t.tile0.size() == sizes.size() + 1);
  uint32_t at = 0;
  bool tail = false;
  for (int b = 0; b < batch; ++b) {
    CHECK(t.tile0[b] == at);
    CHECK(ragged_tiles(sizes[b]) == want_tiles(sizes[b]));
    for (uint32_t i = 0; i < want_tiles(sizes[b]); ++i) {
      CHECK(at + i < t.tile_stripe.size());
      CHECK(t.tile_stripe[at + i] == static_cast<uint32_t>(b));
    }
    at += want_tiles(sizes[b]);
    tail |= sizes[b] % 16 != 0;
  }
  CHECK(t.tile0[batch] == at);
  CHECK(t.ntiles == at);
  CHECK(t.tile_stripe.size() == at);
  CHECK(t.any_tail == tail && t.stripes == batch);
  // the map of a subset: every other stripe included; tile0 is still indexed by stripe
  std::vector<uint8_t> include(sizes.size());
  for (int b = 0; b < batch; ++b) include[b] = b % 2 == 0;
  TileMap u;
  CHECK(build_tile_map(batch, sizes.data(), include.data(), u) == TableError::kOk);
  uint32_t uat = 0;
  bool utail = false;
  for (int b = 0; b < batch; ++b) {
    CHECK(u.tile0[b] == uat);
    if (!include[b]) continue;
    for (uint32_t i = 0; i < want_tiles(sizes[b]); ++i) CHECK(u.tile_stripe.at(uat + i) == static_cast<uint32_t>(b));
    uat += want_tiles(sizes[b]);
    utail |= sizes[b] % 16 != 0;
  }
  CHECK(u.tile0[batch] == uat && u.ntiles == uat && u.tile_stripe.size() == uat);
  CHECK(u.stripes == (batch + 1) / 2 && u.any_tail == utail);
  // every tile covers vectors of its stripe: the last tile of a stripe starts inside it
  for (int b = 0; b < batch; ++b) {
    const uint64_t nvec = sizes[b] / 16;
    const uint32_t last = t.tile0[b + 1] - t.tile0[b] - 1;
    CHECK(last == 0 || static_cast<uint64_t>(last) * kRaggedTileVecs < nvec);
    CHECK(static_cast<uint64_t>(last + 1) * kRaggedTileVecs >= nvec);
  }
  std::printf("tile map of %d stripes: %u tiles ok\n", batch, t.ntiles);
}

void check_tables(int k, int m, int batch, unsigned seed) {
  const int n = k + m;
  std::mt19937 rng(seed);
  std::vector<uint8_t> pres(static_cast<size_t>(batch) * n, 1);
  std::vector<size_t> sizes(static_cast<size_t>(batch));
  for (int b = 0; b < batch; ++b) {
    sizes[b] = 1 + rng() % 40000;
    const int losses = static_cast<int>(rng() % static_cast<unsigned>(m + 1));
    for (int l = 0; l < losses;) {
      const int i = static_cast<int>(rng() % static_cast<unsigned>(n));
      if (pres[static_cast<size_t>(b) * n + i]) {
        pres[static_cast<size_t>(b) * n + i] = 0;
        ++l;
      }
    }
  }
  RaggedTables r;
  MixedTables x;
  CHECK(build_ragged_tables(k, m, batch, sizes.data(), pres.data(), nullptr, r) == TableError::kOk);
  CHECK(build_mixed_tables(k, m, batch, pres.data(), nullptr, x) == TableError::kOk);
  CHECK(r.mixed.k == k && r.mixed.m == m && r.mixed.batch == batch);
  CHECK(r.mixed.pat == x.pat);
  CHECK(r.mixed.P() == x.P());
  for (int p = 0; p < x.P(); ++p) {
    CHECK(r.mixed.patterns[p].mask == x.patterns[p].mask);
    CHECK(r.mixed.patterns[p].valid == x.patterns[p].valid);
    CHECK(r.mixed.patterns[p].rows == x.patterns[p].rows);
    CHECK(r.mixed.patterns[p].missing == x.patterns[p].missing);
  }
  CHECK(r.mixed.groups.size() == x.groups.size());
  for (size_t g = 0; g < x.groups.size(); ++g) {
    CHECK(r.mixed.groups[g].row0 == x.groups[g].row0 && r.mixed.groups[g].R == x.groups[g].R);
    CHECK(r.mixed.groups[g].tab_stride == x.groups[g].tab_stride);
    CHECK(r.mixed.groups[g].arena == x.groups[g].arena);
    CHECK(r.mixed.groups[g].vmask == x.groups[g].vmask);
    CHECK(r.mixed.groups[g].nrows == x.groups[g].nrows);
  }
  // one map shared by every launch group: the one build_tile_map gives for these sizes
  TileMap t;
  CHECK(build_tile_map(batch, sizes.data(), nullptr, t) == TableError::kOk);
  CHECK(r.maps.size() == 1);
  CHECK(r.maps[0].tile0 == t.tile0 && r.maps[0].tile_stripe == t.tile_stripe && r.maps[0].ntiles == t.ntiles);
  CHECK(r.maps[0].any_tail == t.any_tail && r.maps[0].stripes == batch);
  uint64_t total = 0;
  for (int b = 0; b < batch; ++b) {
    CHECK(r.size[b] == sizes[b]);
    total += sizes[b];
  }
  CHECK(r.bytes == total * static_cast<uint64_t>(n));  // every shard of every stripe
  // an all-wanted set that is not null takes the per-group form: the same tables, and every
  // group's map is the shared one
  std::vector<uint8_t> ones(pres.size(), 1);
  RaggedTables q;
  CHECK(build_ragged_tables(k, m, batch, sizes.data(), pres.data(), ones.data(), q) == TableError::kOk);
  CHECK(q.mixed.pat == x.pat && q.bytes == r.bytes && q.size == r.size && q.maps.size() == x.groups.size());
  for (size_t g = 0; g < x.groups.size(); ++g) {
    CHECK(q.mixed.groups[g].arena == x.groups[g].arena && q.mixed.groups[g].vmask == x.groups[g].vmask);
    CHECK(q.maps[g].tile0 == t.tile0 && q.maps[g].tile_stripe == t.tile_stripe && q.maps[g].any_tail == t.any_tail);
  }
  std::printf("RS(%d,%d) batch %d: %d patterns, %u tiles ok\n", k, m, batch, x.P(), r.maps[0].ntiles);
}

}  // namespace

int main() {
  check_map({1, 15, 16, 8191, 8192, 8193, 3 * 8192, 3 * 8192 + 1});
  check_map({3 * 8192 + 1, 1});
  check_map({8192 + 16, 8192 + 15, 16 * 8192 + 5, 7, 2 * 8192 - 1});
  check_map({5});
  {  // the expected map of the first batch, written out
    const std::vector<size_t> sizes = {1, 15, 16, 8191, 8192, 8193, 3 * 8192, 3 * 8192 + 1};
    TileMap t;
    CHECK(build_tile_map(8, sizes.data(), nullptr, t) == TableError::kOk);
    const std::vector<uint32_t> tile0 = {0, 1, 2, 3, 4, 5, 6, 9, 12};
    const std::vector<uint32_t> owner = {0, 1, 2, 3, 4, 5, 6, 6, 6, 7, 7, 7};
    CHECK(t.tile0 == tile0);
    CHECK(t.tile_stripe == owner);
    CHECK(t.ntiles == 12);
  }
  {  // a zero size anywhere
    const std::vector<size_t> sizes = {100, 0, 7};
    TileMap t;
    CHECK(build_tile_map(3, sizes.data(), nullptr, t) == TableError::kNoData);
    std::vector<uint8_t> pres(3 * 14, 1);
    RaggedTables r;
    CHECK(build_ragged_tables(10, 4, 3, sizes.data(), pres.data(), nullptr, r) == TableError::kNoData);
    CHECK(build_ragged_tables(10, 4, 3, sizes.data(), pres.data(), pres.data(), r) == TableError::kNoData);
  }
  if (sizeof(size_t) >= 8) {  // more tiles than a grid holds: reported before anything is sized
    const size_t big = static_cast<size_t>(1) << 44;  // 2^31 tiles
    const std::vector<size_t> one = {big};
    TileMap t;
    CHECK(build_tile_map(1, one.data(), nullptr, t) == TableError::kTooManyTiles);
    const size_t half = static_cast<size_t>(1) << 43;  // 2^30 tiles each
    const std::vector<size_t> two = {half, half - 8192, 16};  // 2^31 - 1 + 1 tiles
    CHECK(build_tile_map(3, two.data(), nullptr, t) == TableError::kTooManyTiles);
    // too many tiles comes before too few shards in a ragged plan's tables
    std::vector<uint8_t> few(3 * 14, 0);
    RaggedTables r;
    CHECK(build_ragged_tables(10, 4, 3, two.data(), few.data(), nullptr, r) == TableError::kTooManyTiles);
    const std::vector<size_t> wrap = {~static_cast<size_t>(0), 17};  // the byte total wraps
    CHECK(build_tile_map(2, wrap.data(), nullptr, t) == TableError::kTooManyTiles);
  }
  {  // too few shards in one stripe
    const std::vector<size_t> sizes = {100, 33, 7};
    std::vector<uint8_t> pres(3 * 14, 1);
    for (int i = 0; i < 5; ++i) pres[14 + i] = 0;
    RaggedTables t;
    CHECK(build_ragged_tables(10, 4, 3, sizes.data(), pres.data(), nullptr, t) == TableError::kTooFewShards);
  }
  {
    const std::vector<size_t> same = {9, 9, 9}, differ = {9, 9, 10};
    CHECK(ragged_sizes_equal(3, same.data()) && !ragged_sizes_equal(3, differ.data()));
    CHECK(ragged_sizes_equal(1, differ.data()));
  }
  check_tables(10, 4, 40, 1);
  check_tables(20, 12, 24, 2);
  std::printf("ragged_host_test ok\n");
  return 0;
}
