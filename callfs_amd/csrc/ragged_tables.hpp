// Host-side tables of a ragged device plan (rs_plan_create_ragged): a batch
// in which every stripe has its own shard size as well as its own presence mask. Patterns,
// arenas and compare masks are those of a mixed plan (mixed_tables.hpp); what a ragged plan
// adds is the tile map. Stripe b is cut into tiles of kRaggedTileVecs 16-byte vectors, at
// least one (a stripe shorter than 16 bytes is one tile whose only work is its S % 16
// tail); tile0 holds the prefix sums and tile_stripe the owning stripe of every tile, so a
// block finds its stripe with one scalar load. Plain C++ with no HIP dependence:
// tests/native/ragged_host_test.cpp builds it with g++ on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "mixed_tables.hpp"

namespace callfs {

constexpr uint64_t kRaggedTileVecs = 512;          // the mixed instances' tile: 8,192 bytes
constexpr uint64_t kRaggedMaxTiles = 0x7fffffffu;  // as launch_mixed bounds its grid

struct RaggedTables {
  MixedTables mixed;                  // patterns, pat[batch], launch groups (arena, vmask)
  std::vector<uint64_t> size;         // [batch] shard bytes of each stripe
  std::vector<uint32_t> tile0;        // [batch + 1] first tile of each stripe; tile0[batch] = ntiles
  std::vector<uint32_t> tile_stripe;  // [ntiles] the stripe that owns each tile
  uint32_t ntiles = 0;
  uint64_t total = 0;   // sum of sizes
  bool any_tail = false;  // some stripe has size % 16 != 0
};

enum class RaggedError { kOk, kNoData, kTooManyTiles, kTooFewShards, kSingular };

// Tiles of a stripe of S shard bytes: ceil(floor(S / 16) / 512), at least 1.
inline uint64_t ragged_tiles(uint64_t S) {
  const uint64_t nvec = S / 16;
  const uint64_t t = (nvec + kRaggedTileVecs - 1) / kRaggedTileVecs;
  return t ? t : 1;
}

// The tile map alone. Sums are 64-bit; a zero size and more than kRaggedMaxTiles tiles (or
// a byte total past 2^64) are reported, and then `t` is left in an unspecified state.
inline RaggedError build_tile_map(int batch, const size_t* sizes, RaggedTables& t) {
  t.size.assign(static_cast<size_t>(batch), 0);
  t.tile0.assign(static_cast<size_t>(batch) + 1, 0);
  t.tile_stripe.clear();
  t.ntiles = 0;
  t.total = 0;
  t.any_tail = false;
  uint64_t ntiles = 0;
  for (int b = 0; b < batch; ++b) {
    const uint64_t S = sizes[b];
    if (S == 0) return RaggedError::kNoData;
    if (t.total + S < t.total) return RaggedError::kTooManyTiles;
    t.total += S;
    t.size[static_cast<size_t>(b)] = S;
    t.tile0[static_cast<size_t>(b)] = static_cast<uint32_t>(ntiles);
    ntiles += ragged_tiles(S);  // < 2^31 + 2^51: no overflow before the check
    if (ntiles > kRaggedMaxTiles) return RaggedError::kTooManyTiles;
    t.any_tail |= (S & 15u) != 0;
  }
  t.tile0[static_cast<size_t>(batch)] = static_cast<uint32_t>(ntiles);
  t.ntiles = static_cast<uint32_t>(ntiles);
  t.tile_stripe.resize(static_cast<size_t>(ntiles));
  for (int b = 0; b < batch; ++b)
    for (uint32_t i = t.tile0[static_cast<size_t>(b)]; i < t.tile0[static_cast<size_t>(b) + 1]; ++i)
      t.tile_stripe[i] = static_cast<uint32_t>(b);
  return RaggedError::kOk;
}

// present: batch * (k + m) flags as for build_mixed_tables. The sizes are checked first (a
// batch with a zero size builds no pattern tables).
inline RaggedError build_ragged_tables(int k, int m, int batch, const size_t* sizes,
                                       const uint8_t* present, RaggedTables& t) {
  const RaggedError e = build_tile_map(batch, sizes, t);
  if (e != RaggedError::kOk) return e;
  switch (build_mixed_tables(k, m, batch, present, t.mixed)) {
    case MixedError::kOk: break;
    case MixedError::kTooFewShards: return RaggedError::kTooFewShards;
    case MixedError::kSingular: return RaggedError::kSingular;
    case MixedError::kRowCount: break;  // the missing-rows form only
  }
  return RaggedError::kOk;
}

// ---- required plans (rs_plan_create_required) ---------------------------
// Patterns with their own row counts (build_mixed_tables_required) leave some stripes with
// no row in a launch group, so every group has a tile map of its own over the stripes that
// have one: tile0 is still indexed by stripe (entries of skipped stripes are never read: no
// tile names them), tile_stripe lists the group's tiles alone. A group no stripe has a row
// in has ntiles = 0 and launches nothing.
struct GroupTileMap {
  std::vector<uint32_t> tile0;        // [batch + 1]
  std::vector<uint32_t> tile_stripe;  // [ntiles]
  uint32_t ntiles = 0;
  int stripes = 0;        // stripes with a row in the group
  bool any_tail = false;  // one of them has size % 16 != 0
};

struct RequiredTables {
  MixedTables mixed;           // build_mixed_tables_required
  std::vector<uint64_t> size;  // [batch]
  std::vector<GroupTileMap> maps;  // one per launch group of `mixed`
  // sum over the stripes with a row of size * (k + written rows + compared rows)
  uint64_t bytes = 0;
};

inline RaggedError build_required_tables(int k, int m, int batch, const size_t* sizes,
                                         const uint8_t* present, const uint8_t* required,
                                         RequiredTables& t) {
  t = RequiredTables();
  t.size.assign(static_cast<size_t>(batch), 0);
  for (int b = 0; b < batch; ++b) {
    if (sizes[b] == 0) return RaggedError::kNoData;
    t.size[static_cast<size_t>(b)] = sizes[b];
  }
  switch (build_mixed_tables_required(k, m, batch, present, required, t.mixed)) {
    case MixedError::kOk: break;
    case MixedError::kTooFewShards: return RaggedError::kTooFewShards;
    case MixedError::kSingular: return RaggedError::kSingular;
    case MixedError::kRowCount: break;  // the missing-rows form only
  }
  for (int b = 0; b < batch; ++b) {
    const uint64_t r = t.mixed.patterns[t.mixed.pat[static_cast<size_t>(b)]].rows.size();
    if (r == 0) continue;
    const uint64_t add = t.size[static_cast<size_t>(b)] * (static_cast<uint64_t>(k) + r);
    if (add / (static_cast<uint64_t>(k) + r) != t.size[static_cast<size_t>(b)] ||
        t.bytes + add < t.bytes)
      return RaggedError::kTooManyTiles;
    t.bytes += add;
  }
  for (const MixedGroup& g : t.mixed.groups) {
    GroupTileMap gm;
    gm.tile0.assign(static_cast<size_t>(batch) + 1, 0);
    uint64_t ntiles = 0;
    for (int b = 0; b < batch; ++b) {
      gm.tile0[static_cast<size_t>(b)] = static_cast<uint32_t>(ntiles);
      if (g.nrows[t.mixed.pat[static_cast<size_t>(b)]] == 0) continue;
      const uint64_t S = t.size[static_cast<size_t>(b)];
      ntiles += ragged_tiles(S);
      if (ntiles > kRaggedMaxTiles) return RaggedError::kTooManyTiles;
      gm.any_tail |= (S & 15u) != 0;
      ++gm.stripes;
    }
    gm.tile0[static_cast<size_t>(batch)] = static_cast<uint32_t>(ntiles);
    gm.ntiles = static_cast<uint32_t>(ntiles);
    gm.tile_stripe.resize(static_cast<size_t>(ntiles));
    for (int b = 0; b < batch; ++b)
      for (uint32_t i = gm.tile0[static_cast<size_t>(b)]; i < gm.tile0[static_cast<size_t>(b) + 1]; ++i)
        gm.tile_stripe[i] = static_cast<uint32_t>(b);
    t.maps.push_back(std::move(gm));
  }
  return RaggedError::kOk;
}

// True when every stripe of the batch has the same shard size.
inline bool ragged_sizes_equal(int batch, const size_t* sizes) {
  for (int b = 1; b < batch; ++b)
    if (sizes[b] != sizes[0]) return false;
  return true;
}

}  // namespace callfs
