// The work list and chunk packing of a heterogeneous host batch (rs_encode_batch /
// rs_reconstruct_batch over stripes of different shard sizes and erasure patterns, DESIGN.md
// §7.5): the call's stripes become items (whole stripes, or column parts of stripes too large
// for a chunk), consecutive items are packed into chunks of at most the chunk budget, and a
// chunk's staging is laid out so that it moves with one H2D and one D2H and runs as one
// ragged launch per launch group (ragged_tables.hpp, "stripe" meaning item). Also the split of
// a call into classes by row count (a reconstruct without verification: by missing count), and
// of a class into segments whose pattern tables stay within kRaggedArenaBudget. Both read the
// kShard* flag rows that admission writes (host_path.hpp). The update and locate routes
// (host_update.hpp, host_locate.hpp) cut their calls with the same ragged_segments over their own
// flag rows and set a run up with the same ragged_shape and RaggedWork. Plain C++ with no HIP
// dependence: tests/native/ragged_chunks_test.cpp builds it with g++ on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "host_path.hpp"
#include "ragged_tables.hpp"

namespace callfs {

// Width of every column part but a stripe's last: a non-zero multiple of one tile of the
// ragged kernels, so parts stay 16-B and 256-B aligned and only the last carries S % 16.
constexpr size_t kRaggedPartBytes = kRaggedTileVecs * 16;  // 8,192
// Pattern tables (all launch groups' arenas) one segment of a call may hold on the device.
constexpr size_t kRaggedArenaBudget = 16u << 20;
// Items per chunk: the grid's y dimension of the in-place kernel.
constexpr size_t kRaggedMaxItems = 65535;

struct RaggedItem {
  int stripe = 0;  // index into the run's stripe list
  size_t off = 0;  // first column
  size_t w = 0;    // columns
};

// One ragged run: stripes that share k and the launch-group structure (rows per pattern).
// nin[b] / nout[b]: the rows stripe b stages as inputs (k, plus its compared shards) and as
// outputs (its missing shards).
struct RaggedShape {
  int k = 0;
  std::vector<int> group_rows;  // R of each launch group
  std::vector<size_t> size;     // [stripes]
  std::vector<int> nin, nout;   // [stripes]
  int stripes() const { return static_cast<int>(size.size()); }
};

// What a checksummed codec batch hashes of a chunk on the device: nothing
// (every other caller), the digest of every shard of an item (an encode: its staged inputs
// and its written rows), or a check of every staged shard against its expected digest (a
// decode: the k inputs and the compared rows). Only whole-stripe items are hashed in a chunk.
enum class SumsMode { kNone, kDigest, kCheck };

inline bool whole_stripe(const RaggedShape& sh, const RaggedItem& it) {
  return it.off == 0 && it.w == sh.size[static_cast<size_t>(it.stripe)];
}
// The rows of a whole-stripe item that are hashed: slots [0, nin) are its staged rows in
// staging order, [nin, nin + nout) its written rows (digest mode alone).
inline size_t sums_rows(const RaggedShape& sh, const RaggedItem& it, SumsMode mode) {
  if (mode == SumsMode::kNone || !whole_stripe(sh, it)) return 0;
  const size_t s = static_cast<size_t>(it.stripe);
  return static_cast<size_t>(sh.nin[s]) + (mode == SumsMode::kDigest ? static_cast<size_t>(sh.nout[s]) : 0);
}

struct ItemLayout {
  size_t in_off = 0;   // input row r at in_off + r * pitch
  size_t out_off = 0;  // output row r at out_off + r * pitch
  size_t pitch = 0;    // round_up(w, 16)
};

// Where everything of one chunk sits in its staging buffer (and, at the same offsets, in the
// device mirror). Input region [0, in_end): the metadata, then every item's input rows.
// Output region [in_end, out_end): the per-item status words, then every item's output rows.
struct ChunkLayout {
  size_t first = 0, count = 0;  // items [first, first + count)
  size_t in_tab_off = 0, pat_off = 0, size_off = 0, tile0_off = 0, tile_stripe_off = 0;
  size_t item_tab_off = 0;  // [count][4] dwords for the in-place kernel (rs_kernels.hpp SmallRaggedArgs)
  std::vector<size_t> out_tab_off;  // per launch group
  size_t meta_end = 0;
  size_t in_end = 0;
  size_t status_off = 0;  // == in_end
  size_t out_end = 0;     // the chunk's total staging
  uint32_t ntiles = 0;
  bool any_tail = false;
  std::vector<ItemLayout> items;  // [count]
  // The regions of sha256_rows (sha256.hpp), absent (sums_count == 0) unless the chunk hashes
  // on the device: the message table in the metadata, the expected digests (check mode) behind
  // the input rows, the digests or flag bytes behind the status words.
  SumsMode sums = SumsMode::kNone;
  size_t sums_count = 0;       // messages = result slots
  size_t sums_tab_off = 0;     // [sums_count][3] dwords
  size_t sums_expect_off = 0;  // [sums_count][32] bytes
  size_t sums_out_off = 0;     // kDigest: [sums_count][32] bytes; kCheck: [sums_count] bytes
  std::vector<uint32_t> sums_slot0;  // [count]: an item's first slot
};

// Lays items [first, first + count) out. with_rows = false: the metadata and status words
// alone (the direct transport, whose rows are the caller's buffers). sums: the regions of a
// chunk that hashes on the device; kNone leaves every offset what it was without them.
inline ChunkLayout layout_chunk(const RaggedShape& sh, const std::vector<RaggedItem>& items,
                                size_t first, size_t count, bool with_rows = true,
                                SumsMode sums = SumsMode::kNone) {
  ChunkLayout L;
  L.first = first;
  L.count = count;
  uint64_t ntiles = 0;
  for (size_t j = 0; j < count; ++j) {
    ntiles += ragged_tiles(items[first + j].w);
    L.any_tail |= (items[first + j].w & 15u) != 0;
  }
  if (sums != SumsMode::kNone) {
    L.sums_slot0.resize(count);
    for (size_t j = 0; j < count; ++j) {
      L.sums_slot0[j] = static_cast<uint32_t>(L.sums_count);
      L.sums_count += sums_rows(sh, items[first + j], sums);
    }
    if (L.sums_count) L.sums = sums;
  }
  L.ntiles = static_cast<uint32_t>(ntiles);
  Packer pk;
  L.in_tab_off = pk.take(sizeof(void*) * count * static_cast<size_t>(sh.k));
  for (int R : sh.group_rows) L.out_tab_off.push_back(pk.take(sizeof(void*) * count * static_cast<size_t>(R)));
  L.pat_off = pk.take(sizeof(uint32_t) * count);
  L.size_off = pk.take(sizeof(uint64_t) * count);
  L.tile0_off = pk.take(sizeof(uint32_t) * (count + 1));
  L.tile_stripe_off = pk.take(sizeof(uint32_t) * static_cast<size_t>(ntiles));
  L.item_tab_off = pk.take(4 * sizeof(uint32_t) * count);
  if (L.sums_count) L.sums_tab_off = pk.take(3 * sizeof(uint32_t) * L.sums_count);
  L.meta_end = pk.off;
  L.items.resize(count);
  for (size_t j = 0; j < count; ++j) {
    const RaggedItem& it = items[first + j];
    L.items[j].pitch = round_up(it.w, 16);
    if (with_rows) L.items[j].in_off = pk.take(L.items[j].pitch * static_cast<size_t>(sh.nin[it.stripe]));
  }
  if (L.sums == SumsMode::kCheck) L.sums_expect_off = pk.take(32 * L.sums_count);
  L.in_end = L.status_off = pk.off;
  pk.take(sizeof(int) * count);
  if (L.sums_count) L.sums_out_off = pk.take((L.sums == SumsMode::kDigest ? 32 : 1) * L.sums_count);
  for (size_t j = 0; j < count; ++j) {
    const RaggedItem& it = items[first + j];
    if (with_rows) L.items[j].out_off = pk.take(L.items[j].pitch * static_cast<size_t>(sh.nout[it.stripe]));
  }
  L.out_end = pk.off;
  return L;
}

// Staging of a chunk that holds the one item (stripe b, w columns).
inline size_t single_item_bytes(const RaggedShape& sh, int b, size_t w) {
  std::vector<RaggedItem> one(1);
  one[0].stripe = b;
  one[0].w = w;
  return layout_chunk(sh, one, 0, 1).out_end;
}

// The budget chunks are held to: `budget`, or what one item of one tile's width needs when
// that is more (k + m shards of 8,192 bytes do not fit a 64 KiB chunk for k + m > 7: a
// part cannot be narrower than one tile, so such a chunk holds one item and exceeds
// `budget`).
inline size_t ragged_effective_budget(const RaggedShape& sh, size_t budget) {
  size_t need = 0;
  for (int b = 0; b < sh.stripes(); ++b)
    need = std::max(need, single_item_bytes(sh, b, std::min(sh.size[b], kRaggedPartBytes)));
  return std::max(budget, need);
}

// The run's items in stripe order. A stripe whose staging fits a chunk is one item; a larger
// one is cut into parts of the widest multiple of kRaggedPartBytes that fits (the last part
// takes the rest).
inline std::vector<RaggedItem> ragged_items(const RaggedShape& sh, size_t budget) {
  const size_t eff = ragged_effective_budget(sh, budget);
  std::vector<RaggedItem> items;
  for (int b = 0; b < sh.stripes(); ++b) {
    const size_t S = sh.size[b];
    if (single_item_bytes(sh, b, S) <= eff) {
      items.push_back({b, 0, S});
      continue;
    }
    // widest part: staging grows with w, so bisect over multiples of the part width
    size_t lo = 1, hi = S / kRaggedPartBytes;  // in parts; lo always fits (eff covers one tile)
    while (lo < hi) {
      const size_t mid = (lo + hi + 1) / 2;
      if (single_item_bytes(sh, b, mid * kRaggedPartBytes) <= eff) lo = mid;
      else hi = mid - 1;
    }
    const size_t cw = lo * kRaggedPartBytes;
    for (size_t off = 0; off < S; off += cw) items.push_back({b, off, std::min(cw, S - off)});
  }
  return items;
}

// Packs consecutive items into chunks: as many as fit `budget` (and kRaggedMaxItems), at
// least one (an item alone may need up to ragged_effective_budget). Returns the chunks'
// layouts in order.
inline std::vector<ChunkLayout> ragged_chunks(const RaggedShape& sh, const std::vector<RaggedItem>& items,
                                              size_t budget, bool with_rows = true,
                                              SumsMode sums = SumsMode::kNone) {
  std::vector<ChunkLayout> chunks;
  size_t first = 0;
  while (first < items.size()) {
    // staging grows with the item count: gallop, then bisect
    size_t lo = 1, hi = std::min(items.size() - first, kRaggedMaxItems);
    size_t step = 1;
    while (lo < hi) {
      const size_t probe = std::min(hi, lo + step);
      if (layout_chunk(sh, items, first, probe, with_rows, sums).out_end <= budget) {
        lo = probe;
        step *= 2;
      } else {
        hi = probe - 1;
        break;
      }
    }
    while (lo < hi) {
      const size_t mid = (lo + hi + 1) / 2;
      if (layout_chunk(sh, items, first, mid, with_rows, sums).out_end <= budget) lo = mid;
      else hi = mid - 1;
    }
    chunks.push_back(layout_chunk(sh, items, first, lo, with_rows, sums));
    first += lo;
  }
  return chunks;
}

// The shape of a run: k pointer slots per item, the launch groups' rows, the stripes' sizes and,
// from rows_of(s) = {nin, nout}, the rows stripe s stages.
template <class Groups, class RowsF>
RaggedShape ragged_shape(int k, const Groups& groups, std::vector<size_t> sizes, RowsF rows_of) {
  RaggedShape sh;
  sh.k = k;
  for (const auto& g : groups) sh.group_rows.push_back(g.R);
  sh.size = std::move(sizes);
  for (int s = 0; s < sh.stripes(); ++s) {
    const std::pair<int, int> rows = rows_of(s);
    sh.nin.push_back(rows.first);
    sh.nout.push_back(rows.second);
  }
  return sh;
}

// A run's work list: its items, and once cut() its chunks.
struct RaggedWork {
  std::vector<RaggedItem> items;
  std::vector<ChunkLayout> chunks;
  RaggedWork(const RaggedShape& sh, size_t budget) : items(ragged_items(sh, budget)) {}
  // Packs the items into chunks; false where a chunk has more tiles than a launch's grid holds.
  bool cut(const RaggedShape& sh, size_t budget, SumsMode sums = SumsMode::kNone) {
    chunks = ragged_chunks(sh, items, budget, true, sums);
    for (const ChunkLayout& C : chunks)
      if (C.ntiles > kRaggedMaxTiles) return false;
    return true;
  }
};

// The part of a chunk's metadata every tile-map kernel reads, at `h` (the start of its
// staging): the items' sizes and the tile map over them.
inline void fill_chunk_tile_map(const ChunkLayout& L, const std::vector<RaggedItem>& items, uint8_t* h) {
  std::vector<size_t> widths(L.count);
  auto* size = reinterpret_cast<uint64_t*>(h + L.size_off);
  for (size_t j = 0; j < L.count; ++j) size[j] = widths[j] = items[L.first + j].w;
  TileMap tm;
  (void)build_tile_map(static_cast<int>(L.count), widths.data(), nullptr, tm);
  std::memcpy(h + L.tile0_off, tm.tile0.data(), sizeof(uint32_t) * tm.tile0.size());
  std::memcpy(h + L.tile_stripe_off, tm.tile_stripe.data(), sizeof(uint32_t) * tm.tile_stripe.size());
}

// Fills a chunk's metadata at `h` (the start of its staging). stripe_pat[b]: the pattern of
// the run's stripe b in `mt`. in_ptr(j, i): the address the kernels read item j's input i
// (the pattern's valid[i]) at; row_ptr(j, r): that of its row r (rows[r]: written for
// r < missing, compared beyond).
template <class InP, class RowP>
void fill_chunk_meta(const ChunkLayout& L, const RaggedShape& sh, const std::vector<RaggedItem>& items,
                     const MixedTables& mt, const uint32_t* stripe_pat, uint8_t* h, InP in_ptr,
                     RowP row_ptr) {
  const size_t k = static_cast<size_t>(sh.k);
  auto* in = reinterpret_cast<const uint8_t**>(h + L.in_tab_off);
  auto* pat = reinterpret_cast<uint32_t*>(h + L.pat_off);
  for (size_t j = 0; j < L.count; ++j) {
    pat[j] = stripe_pat[items[L.first + j].stripe];
    for (size_t i = 0; i < k; ++i) in[j * k + i] = in_ptr(j, static_cast<int>(i));
  }
  for (size_t gi = 0; gi < mt.groups.size(); ++gi) {
    const MixedGroup& g = mt.groups[gi];
    auto* out = reinterpret_cast<uint8_t**>(h + L.out_tab_off[gi]);
    for (size_t j = 0; j < L.count; ++j)
      for (int r = 0; r < g.R; ++r) out[j * g.R + r] = row_ptr(j, g.row0 + r);
  }
  fill_chunk_tile_map(L, items, h);
  auto* tab = reinterpret_cast<uint32_t*>(h + L.item_tab_off);
  for (size_t j = 0; j < L.count; ++j) {
    tab[4 * j + 0] = static_cast<uint32_t>(L.items[j].in_off / 16);
    tab[4 * j + 1] = static_cast<uint32_t>(L.items[j].out_off / 16);
    tab[4 * j + 2] = static_cast<uint32_t>(items[L.first + j].w);
    tab[4 * j + 3] = pat[j];
  }
  std::memset(h + L.status_off, 0, sizeof(int) * L.count);
}

// A stripe's flag is the OR of its items' flags. Returns true when any was set.
inline bool fold_item_status(const ChunkLayout& L, const std::vector<RaggedItem>& items,
                             const int* item_status, int* stripe_flags) {
  bool any = false;
  for (size_t j = 0; j < L.count; ++j)
    if (item_status[j]) {
      any = true;
      stripe_flags[items[L.first + j].stripe] = 1;
    }
  return any;
}

// The stripes of a call by class: one class per row count r = wanted missing shards + (verify:
// present shards beyond the first k), in ascending r, so that every pattern of a class has
// exactly r rows, which is what the ragged kernels rest on; `rows` holds r. Stripes with r = 0
// are in no class. flags: stripes * n of kShard* (host_path.hpp). Where every missing shard is
// wanted, verify gives r = m for every stripe (one class: encodes, verify != 0) and !verify
// gives r = the missing count (a reconstruct with verify == 0).
struct RaggedClass {
  int rows = 0;
  std::vector<int> stripes;
};
inline std::vector<RaggedClass> ragged_classes(int n, int k, int stripes, const uint8_t* flags, bool verify) {
  std::vector<std::vector<int>> by(static_cast<size_t>(n) + 1);
  for (int b = 0; b < stripes; ++b) {
    int w = 0, np = 0;
    for (int i = 0; i < n; ++i) {
      w += flags[static_cast<size_t>(b) * n + i] == kShardWanted;
      np += flags[static_cast<size_t>(b) * n + i] == kShardPresent;
    }
    by[static_cast<size_t>(w + (verify && np > k ? np - k : 0))].push_back(b);
  }
  std::vector<RaggedClass> out;
  for (int r = 1; r <= n; ++r)
    if (!by[r].empty()) out.push_back({r, std::move(by[r])});
  return out;
}

// Bytes of one pattern's tables over every launch group of `rows` rows.
inline size_t pattern_arena_bytes(int k, int rows) {
  size_t bytes = 0;
  for (int g0 = 0; g0 < rows; g0 += kMixedRowsPerLaunch)
    bytes += static_cast<size_t>(k) * 32u * nibble_width(std::min(kMixedRowsPerLaunch, rows - g0));
  return bytes;
}

// Cuts a stripe list into segments [begin, end) of consecutive entries whose distinct patterns'
// tables stay within `budget` (one pattern always fits). A pattern is a stripe's whole flag row,
// `width` bytes at flags + stripe * width, and costs `per` bytes of tables.
inline std::vector<std::pair<size_t, size_t>> ragged_segments(size_t width, size_t per,
                                                              const std::vector<int>& stripes,
                                                              const uint8_t* flags, size_t budget) {
  const size_t max_patterns = std::max<size_t>(1, budget / std::max<size_t>(per, 1));
  std::vector<std::pair<size_t, size_t>> segs;
  std::set<std::string> seen;
  size_t begin = 0;
  for (size_t j = 0; j < stripes.size(); ++j) {
    std::string key(reinterpret_cast<const char*>(flags + static_cast<size_t>(stripes[j]) * width), width);
    if (!seen.count(key) && seen.size() == max_patterns) {
      segs.push_back({begin, j});
      begin = j;
      seen.clear();
    }
    seen.insert(std::move(key));
  }
  if (begin < stripes.size()) segs.push_back({begin, stripes.size()});
  return segs;
}
// A class of the ragged route: the pattern is the row of n kShard* flags (the mask and the
// wanted missing shards), its tables those of `rows` rows.
inline std::vector<std::pair<size_t, size_t>> ragged_segments(int k, int n, int rows,
                                                              const std::vector<int>& stripes,
                                                              const uint8_t* flags, size_t budget) {
  return ragged_segments(static_cast<size_t>(n), pattern_arena_bytes(k, rows), stripes, flags, budget);
}

}  // namespace callfs
