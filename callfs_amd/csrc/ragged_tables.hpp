// Host-side tables of a ragged device plan (rs_plan_create_ragged) and of a
// required one (rs_plan_create_required, §5.10): a batch in which every stripe has its own
// shard size as well as its own pattern. Patterns, arenas and compare masks are those of a
// mixed plan (mixed_tables.hpp); what these plans add is the tile map. A stripe is cut into
// tiles of kRaggedTileVecs 16-byte vectors, at least one (a stripe shorter than 16 bytes is
// one tile whose only work is its S % 16 tail); tile0 holds the prefix sums and tile_stripe
// the owning stripe of every tile, so a block finds its stripe with one scalar load. A ragged
// plan (every pattern has m rows) has one map over all stripes, shared by its launch groups; a
// required plan (patterns with their own row counts) has one map per launch group, over the
// stripes with a row in it. Plain C++ with no HIP dependence:
// tests/native/ragged_host_test.cpp and required_host_test.cpp build it with g++ on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "mixed_tables.hpp"

namespace callfs {

constexpr uint64_t kRaggedTileVecs = 512;          // the mixed instances' tile: 8,192 bytes
constexpr uint64_t kRaggedMaxTiles = 0x7fffffffu;  // as launch_mixed bounds its grid

// tile0 is indexed by stripe whichever stripes the map includes (entries of skipped stripes
// are never read: no tile names them); tile_stripe lists the included stripes' tiles alone.
struct TileMap {
  std::vector<uint32_t> tile0;        // [batch + 1] first tile of each stripe; tile0[batch] = ntiles
  std::vector<uint32_t> tile_stripe;  // [ntiles] the stripe that owns each tile
  uint32_t ntiles = 0;
  int stripes = 0;        // stripes included
  bool any_tail = false;  // one of them has size % 16 != 0
};

struct RaggedTables {
  MixedTables mixed;           // patterns, pat[batch], launch groups (arena, vmask, nrows)
  std::vector<uint64_t> size;  // [batch] shard bytes of each stripe
  // one map shared by every launch group (a ragged plan), or one per launch group of `mixed`
  // (a required plan); a group no stripe has a row in has ntiles = 0 and launches nothing
  std::vector<TileMap> maps;
  // sum over the stripes with a row of size * (k + written rows + compared rows)
  uint64_t bytes = 0;
};

// Tiles of a stripe of S shard bytes: ceil(floor(S / 16) / 512), at least 1.
inline uint64_t ragged_tiles(uint64_t S) {
  const uint64_t nvec = S / 16;
  const uint64_t t = (nvec + kRaggedTileVecs - 1) / kRaggedTileVecs;
  return t ? t : 1;
}

// The tile map over the stripes whose `include` flag is set (null: every stripe). A zero size
// and more than kRaggedMaxTiles tiles are reported, and then `t` is left in an unspecified
// state.
inline TableError build_tile_map(int batch, const size_t* sizes, const uint8_t* include, TileMap& t) {
  t = TileMap();
  t.tile0.assign(static_cast<size_t>(batch) + 1, 0);
  uint64_t ntiles = 0;
  for (int b = 0; b < batch; ++b) {
    const uint64_t S = sizes[b];
    if (S == 0) return TableError::kNoData;
    t.tile0[static_cast<size_t>(b)] = static_cast<uint32_t>(ntiles);
    if (include && !include[b]) continue;
    ntiles += ragged_tiles(S);  // < 2^31 + 2^51: no overflow before the check
    if (ntiles > kRaggedMaxTiles) return TableError::kTooManyTiles;
    t.any_tail |= (S & 15u) != 0;
    ++t.stripes;
  }
  t.tile0[static_cast<size_t>(batch)] = static_cast<uint32_t>(ntiles);
  t.ntiles = static_cast<uint32_t>(ntiles);
  t.tile_stripe.resize(static_cast<size_t>(ntiles));
  for (int b = 0; b < batch; ++b)
    for (uint32_t i = t.tile0[static_cast<size_t>(b)]; i < t.tile0[static_cast<size_t>(b) + 1]; ++i)
      t.tile_stripe[i] = static_cast<uint32_t>(b);
  return TableError::kOk;
}

// present, required: batch * (k + m) flags as for build_mixed_tables. The sizes are checked
// first (a batch with a zero size builds no pattern tables). required null (every missing shard
// wanted, so every stripe has a row in every launch group): the one map over all stripes, built
// before the pattern tables. Otherwise one map per launch group after them, so the tile limit
// is counted over the stripes that have a row.
inline TableError build_ragged_tables(int k, int m, int batch, const size_t* sizes,
                                      const uint8_t* present, const uint8_t* required,
                                      RaggedTables& t) {
  t = RaggedTables();
  t.size.assign(static_cast<size_t>(batch), 0);
  for (int b = 0; b < batch; ++b) {
    if (sizes[b] == 0) return TableError::kNoData;
    t.size[static_cast<size_t>(b)] = sizes[b];
  }
  if (!required) {
    t.maps.resize(1);
    const TableError e = build_tile_map(batch, sizes, nullptr, t.maps[0]);
    if (e != TableError::kOk) return e;
  }
  const TableError me = build_mixed_tables(k, m, batch, present, required, t.mixed);
  if (me != TableError::kOk) return me;
  for (int b = 0; b < batch; ++b) {
    const uint64_t r = t.mixed.patterns[t.mixed.pat[static_cast<size_t>(b)]].rows.size();
    if (r == 0) continue;
    uint64_t add;
    if (__builtin_mul_overflow(t.size[static_cast<size_t>(b)], static_cast<uint64_t>(k) + r, &add) ||
        __builtin_add_overflow(t.bytes, add, &t.bytes))
      return TableError::kTooManyTiles;
  }
  if (!required) return TableError::kOk;
  std::vector<uint8_t> include(static_cast<size_t>(batch));
  for (const MixedGroup& g : t.mixed.groups) {
    for (int b = 0; b < batch; ++b)
      include[static_cast<size_t>(b)] = g.nrows[t.mixed.pat[static_cast<size_t>(b)]] != 0;
    t.maps.emplace_back();
    const TableError e = build_tile_map(batch, sizes, include.data(), t.maps.back());
    if (e != TableError::kOk) return e;
  }
  return TableError::kOk;
}

// True when every stripe of the batch has the same shard size.
inline bool ragged_sizes_equal(int batch, const size_t* sizes) {
  for (int b = 1; b < batch; ++b)
    if (sizes[b] != sizes[0]) return false;
  return true;
}

}  // namespace callfs
