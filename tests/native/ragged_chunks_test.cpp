// The work list and chunk packing of heterogeneous host batches
// (callfs_amd/csrc/ragged_chunks.hpp) on the CPU, built with g++ -fsanitize=address,undefined
// by tests/test_native_ragged_chunks.py. Over seeded size lists, budgets of 64 KiB and
// 16 MiB and n = 6 and n = 30: every (stripe, byte) lies in exactly one item; every part but
// a stripe's last is a non-zero multiple of 8,192 wide; every chunk is within the budget and
// every item fits one; item starts are 256-B aligned, pitches round_up(w, 16), no two rows
// overlap; the input rows form one range that holds the metadata, the output rows and status
// words a second one disjoint from it; the tile map equals build_tile_map of the items'
// widths; part flags fold onto the right stripe; the verify == 0 classes partition the stripes
// by missing count and their patterns have that many rows; segments respect the arena budget;
// all-wanted flag rows give the classes and segment cuts of a call without a wanted set.
//
// The budget: a part cannot be narrower than one 8,192-byte tile, and n shards of 8,192 bytes
// plus metadata exceed 64 KiB for n > 7. There the bound that can hold is the staging of one
// tile-wide item (ragged_effective_budget), and such chunks hold exactly one item; wherever
// one tile-wide item fits `budget` (n = 6 at 64 KiB, both n at 16 MiB) the bound is `budget`
// itself, which check_run asserts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "gf256.hpp"
#include "mixed_tables.hpp"
#include "ragged_chunks.hpp"
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

struct Range {
  size_t lo, hi;
};

// masks of `stripes` stripes of RS(k, m): between 0 and m shards missing each
std::vector<uint8_t> random_masks(int k, int m, int stripes, std::mt19937& rng, int min_missing) {
  const int n = k + m;
  std::vector<uint8_t> pres(static_cast<size_t>(stripes) * n, 1);
  for (int b = 0; b < stripes; ++b) {
    const int e = min_missing + static_cast<int>(rng() % static_cast<unsigned>(m - min_missing + 1));
    for (int j = 0; j < e;) {
      const int i = static_cast<int>(rng() % static_cast<unsigned>(n));
      if (pres[static_cast<size_t>(b) * n + i]) {
        pres[static_cast<size_t>(b) * n + i] = 0;
        ++j;
      }
    }
  }
  return pres;
}

// one run (every stripe of `sizes` with masks `pres`; rows = m with compares, or e missing
// only) at `budget`
void check_run(int k, int m, int rows, bool missing_only, const std::vector<size_t>& sizes,
               const std::vector<uint8_t>& pres, size_t budget) {
  const int n = k + m, stripes = static_cast<int>(sizes.size());
  MixedTables mt;
  CHECK(build_mixed_tables(k, m, stripes, pres.data(), nullptr, mt, !missing_only) == TableError::kOk);
  CHECK(mt.rows == rows && mixed_rows_are(mt, rows));
  RaggedShape sh;
  sh.k = k;
  for (const MixedGroup& g : mt.groups) sh.group_rows.push_back(g.R);
  for (int b = 0; b < stripes; ++b) {
    const MixedPattern& pt = mt.patterns[mt.pat[b]];
    CHECK(static_cast<int>(pt.rows.size()) == rows);
    sh.size.push_back(sizes[b]);
    sh.nin.push_back(k + rows - pt.missing);
    sh.nout.push_back(pt.missing);
  }
  const size_t eff = ragged_effective_budget(sh, budget);
  // the budget itself wherever one tile-wide item of n shards fits it
  if (static_cast<size_t>(n) * kRaggedPartBytes + 8192 <= budget) CHECK(eff == budget);
  const std::vector<RaggedItem> items = ragged_items(sh, budget);

  // every (stripe, byte) in exactly one item, in stripe order; part widths
  size_t at = 0;
  for (int b = 0; b < stripes; ++b) {
    size_t col = 0;
    while (col < sizes[b]) {
      CHECK(at < items.size());
      const RaggedItem& it = items[at];
      CHECK(it.stripe == b && it.off == col && it.w > 0 && it.off + it.w <= sizes[b]);
      if (it.off + it.w < sizes[b]) CHECK(it.w % kRaggedPartBytes == 0);
      CHECK(single_item_bytes(sh, b, it.w) <= eff);
      col += it.w;
      ++at;
    }
  }
  CHECK(at == items.size());

  const std::vector<ChunkLayout> chunks = ragged_chunks(sh, items, budget);
  size_t next = 0;
  std::vector<int> flags(static_cast<size_t>(stripes), 0), want(static_cast<size_t>(stripes), 0);
  for (const ChunkLayout& C : chunks) {
    CHECK(C.first == next && C.count >= 1);
    next += C.count;
    CHECK(C.out_end <= eff);
    if (C.out_end > budget) CHECK(C.count == 1);
    // a chunk holds as many items as fit
    if (next < items.size() && C.count < kRaggedMaxItems)
      CHECK(layout_chunk(sh, items, C.first, C.count + 1).out_end > budget);
    CHECK(C.items.size() == C.count);
    CHECK(C.status_off == C.in_end && C.meta_end <= C.in_end && C.in_end < C.out_end);
    std::vector<Range> rows_in, rows_out, all;
    // the metadata pieces
    std::vector<Range> meta = {{C.in_tab_off, C.in_tab_off + 8 * C.count * k},
                               {C.pat_off, C.pat_off + 4 * C.count},
                               {C.size_off, C.size_off + 8 * C.count},
                               {C.tile0_off, C.tile0_off + 4 * (C.count + 1)},
                               {C.tile_stripe_off, C.tile_stripe_off + 4 * static_cast<size_t>(C.ntiles)},
                               {C.item_tab_off, C.item_tab_off + 16 * C.count}};
    CHECK(C.out_tab_off.size() == mt.groups.size());
    for (size_t gi = 0; gi < mt.groups.size(); ++gi)
      meta.push_back({C.out_tab_off[gi], C.out_tab_off[gi] + 8 * C.count * mt.groups[gi].R});
    for (const Range& r : meta) {
      CHECK(r.lo % 256 == 0 && r.hi <= C.meta_end);
      all.push_back(r);
    }
    all.push_back({C.status_off, C.status_off + 4 * C.count});
    std::vector<size_t> widths;
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      widths.push_back(it.w);
      CHECK(il.pitch == round_up(it.w, 16));
      CHECK(il.in_off % 256 == 0 && il.out_off % 256 == 0);
      for (int r = 0; r < sh.nin[it.stripe]; ++r) rows_in.push_back({il.in_off + il.pitch * r, il.in_off + il.pitch * (r + 1)});
      for (int r = 0; r < sh.nout[it.stripe]; ++r) rows_out.push_back({il.out_off + il.pitch * r, il.out_off + il.pitch * (r + 1)});
    }
    // the input rows lie in [meta_end, in_end) of the input region [0, in_end), which holds
    // the metadata; the status words and output rows in [in_end, out_end)
    for (const Range& r : rows_in) {
      CHECK(r.lo >= C.meta_end && r.hi <= C.in_end);
      all.push_back(r);
    }
    for (const Range& r : rows_out) {
      CHECK(r.lo >= C.status_off + 4 * C.count && r.hi <= C.out_end);
      all.push_back(r);
    }
    std::sort(all.begin(), all.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    for (size_t i = 1; i < all.size(); ++i) CHECK(all[i - 1].hi <= all[i].lo);

    // the filled metadata: the tile map of the items' widths, pointers, item table
    std::vector<uint8_t> h(C.out_end, 0xEE);
    uint8_t* base = reinterpret_cast<uint8_t*>(uintptr_t(1) << 40);
    fill_chunk_meta(C, sh, items, mt, mt.pat.data(), h.data(),
                    [&](size_t j, int i) { return base + C.items[j].in_off + C.items[j].pitch * i; },
                    [&](size_t j, int row) { return base + 1 + j * 1000 + row; });
    TileMap tm;
    CHECK(build_tile_map(static_cast<int>(C.count), widths.data(), nullptr, tm) == TableError::kOk);
    CHECK(tm.ntiles == C.ntiles && tm.any_tail == C.any_tail);
    const std::vector<uint64_t> size64(widths.begin(), widths.end());
    CHECK(std::memcmp(h.data() + C.size_off, size64.data(), 8 * C.count) == 0);
    CHECK(std::memcmp(h.data() + C.tile0_off, tm.tile0.data(), 4 * (C.count + 1)) == 0);
    CHECK(std::memcmp(h.data() + C.tile_stripe_off, tm.tile_stripe.data(), 4 * static_cast<size_t>(C.ntiles)) == 0);
    const auto* in = reinterpret_cast<uint8_t* const*>(h.data() + C.in_tab_off);
    const auto* pat = reinterpret_cast<const uint32_t*>(h.data() + C.pat_off);
    const auto* tab = reinterpret_cast<const uint32_t*>(h.data() + C.item_tab_off);
    const auto* st = reinterpret_cast<const int*>(h.data() + C.status_off);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      CHECK(pat[j] == mt.pat[it.stripe] && st[j] == 0);
      for (int i = 0; i < k; ++i) CHECK(in[j * k + i] == base + C.items[j].in_off + C.items[j].pitch * i);
      CHECK(tab[4 * j] * 16ull == C.items[j].in_off && tab[4 * j + 1] * 16ull == C.items[j].out_off);
      CHECK(tab[4 * j + 2] == it.w && tab[4 * j + 3] == pat[j]);
    }
    for (size_t gi = 0; gi < mt.groups.size(); ++gi) {
      const auto* out = reinterpret_cast<uint8_t* const*>(h.data() + C.out_tab_off[gi]);
      const int R = mt.groups[gi].R;
      for (size_t j = 0; j < C.count; ++j)
        for (int r = 0; r < R; ++r) CHECK(out[j * R + r] == base + 1 + j * 1000 + mt.groups[gi].row0 + r);
    }
    // flags of parts fold onto their stripe: flag every third item of the chunk
    std::vector<int> item_status(C.count, 0);
    for (size_t j = 0; j < C.count; j += 3) {
      item_status[j] = 1;
      want[items[C.first + j].stripe] = 1;
    }
    CHECK(fold_item_status(C, items, item_status.data(), flags.data()));
  }
  CHECK(next == items.size());
  CHECK(flags == want);
}

void check_classes_and_segments(int k, int m, std::mt19937& rng) {
  const int n = k + m, stripes = 40;
  const std::vector<uint8_t> pres = random_masks(k, m, stripes, rng, 0);
  // with compares: one class of every stripe
  auto one = ragged_classes(n, k, stripes, pres.data(), true);
  CHECK(one.size() == 1 && static_cast<int>(one[0].stripes.size()) == stripes && one[0].rows == m);
  // verify == 0: a partition of the stripes with something missing, by missing count
  auto cls = ragged_classes(n, k, stripes, pres.data(), false);
  std::vector<int> seen(stripes, 0);
  int last_e = 0;
  for (const RaggedClass& c : cls) {
    CHECK(c.rows > last_e && !c.stripes.empty());
    last_e = c.rows;
    std::vector<uint8_t> sub;
    for (int b : c.stripes) {
      int e = 0;
      for (int i = 0; i < n; ++i) e += !pres[static_cast<size_t>(b) * n + i];
      CHECK(e == c.rows);
      CHECK(!seen[b]++);
      sub.insert(sub.end(), pres.begin() + static_cast<size_t>(b) * n, pres.begin() + static_cast<size_t>(b + 1) * n);
    }
    MixedTables mt;
    CHECK(build_mixed_tables(k, m, static_cast<int>(c.stripes.size()), sub.data(), nullptr, mt, false) == TableError::kOk);
    CHECK(mixed_rows_are(mt, c.rows));
    int grows = 0;
    for (const MixedGroup& g : mt.groups) {
      grows += g.R;
      for (uint32_t v : g.vmask) CHECK(v == 0);  // every row written
      CHECK(g.arena.size() == mt.patterns.size() * g.tab_stride);
    }
    CHECK(grows == c.rows);
    for (const MixedPattern& p : mt.patterns) CHECK(static_cast<int>(p.rows.size()) == c.rows && p.missing == c.rows);
    // the rows are those of the full tables' missing rows
    MixedTables full;
    CHECK(build_mixed_tables(k, m, static_cast<int>(c.stripes.size()), sub.data(), nullptr, full) == TableError::kOk);
    CHECK(full.rows == m && full.patterns.size() == mt.patterns.size());
    for (size_t p = 0; p < mt.patterns.size(); ++p)
      for (int r = 0; r < c.rows; ++r) {
        CHECK(mt.patterns[p].rows[r] == full.patterns[p].rows[r]);
        const MixedGroup& a = mt.groups[r / 16];
        const MixedGroup& b = full.groups[r / 16];
        const size_t Wa = nibble_width(a.R), Wb = nibble_width(b.R);
        for (int i = 0; i < k; ++i)  // the coefficient: entry 1 of the low nibble table
          CHECK(a.arena[p * a.tab_stride + i * 32 * Wa + Wa + r % 16] == b.arena[p * b.tab_stride + i * 32 * Wb + Wb + r % 16]);
      }
    // a wrong missing count is refused
    CHECK(build_mixed_tables(k, m, 1, sub.data(), nullptr, mt, false) == TableError::kOk);
    CHECK(mixed_rows_are(mt, c.rows) && !mixed_rows_are(mt, c.rows + 1) && !mixed_rows_are(mt, c.rows - 1));
  }
  for (int b = 0; b < stripes; ++b) {
    int e = 0;
    for (int i = 0; i < n; ++i) e += !pres[static_cast<size_t>(b) * n + i];
    CHECK(seen[b] == (e > 0));
  }
  // segments: consecutive, covering, distinct patterns within the budget
  std::vector<int> all(stripes);
  for (int b = 0; b < stripes; ++b) all[b] = b;
  const size_t per = pattern_arena_bytes(k, m);
  for (size_t budget : {per, 3 * per + 1, size_t(kRaggedArenaBudget)}) {
    const auto segs = ragged_segments(k, n, m, all, pres.data(), budget);
    size_t at = 0;
    for (const auto& s : segs) {
      CHECK(s.first == at && s.second > s.first);
      at = s.second;
      std::map<std::vector<uint8_t>, int> distinct;
      for (size_t j = s.first; j < s.second; ++j)
        distinct[std::vector<uint8_t>(pres.begin() + all[j] * n, pres.begin() + (all[j] + 1) * n)] = 1;
      CHECK(distinct.size() * per <= std::max(budget, per));
      // the tables built over the segment are what the bound speaks of
      std::vector<uint8_t> sub(pres.begin() + s.first * n, pres.begin() + s.second * n);
      MixedTables mt;
      CHECK(build_mixed_tables(k, m, static_cast<int>(s.second - s.first), sub.data(), nullptr, mt) == TableError::kOk);
      size_t arena = 0;
      for (const MixedGroup& g : mt.groups) arena += g.arena.size();
      CHECK(arena == distinct.size() * per);
    }
    CHECK(at == static_cast<size_t>(stripes));
  }
}

// Flag rows that hold kShardWanted / kShardPresent alone (a plain 0 / 1 mask: every missing
// shard wanted) give the classes and segments of a call without a wanted set. The expectation
// is written out from those rules: with compares one class of every stripe (each has m rows);
// without, one class per missing count in ascending order, stripes in call order, none for a
// complete stripe; a segment ends before the stripe whose mask would be one distinct mask more
// than max(1, budget / bytes per pattern).
void check_all_wanted_rules(int k, int m, std::mt19937& rng) {
  const int n = k + m, stripes = 60;
  std::vector<uint8_t> pres = random_masks(k, m, stripes, rng, 0);
  for (int b = 10; b < stripes; b += 3) {  // repeats of earlier masks
    const int src = static_cast<int>(rng() % static_cast<unsigned>(b));
    std::copy(pres.begin() + src * n, pres.begin() + (src + 1) * n, pres.begin() + b * n);
  }
  static_assert(kShardWanted == 0 && kShardPresent == 1, "a 0 / 1 mask is a flag row");
  auto missing = [&](int b) {
    int e = 0;
    for (int i = 0; i < n; ++i) e += pres[static_cast<size_t>(b) * n + i] == 0;
    return e;
  };
  const auto with = ragged_classes(n, k, stripes, pres.data(), true);
  CHECK(with.size() == 1 && with[0].rows == m);
  for (int b = 0; b < stripes; ++b) CHECK(with[0].stripes.at(b) == b);
  std::vector<std::pair<int, std::vector<int>>> want;
  for (int e = 1; e <= n; ++e) {
    std::vector<int> ids;
    for (int b = 0; b < stripes; ++b)
      if (missing(b) == e) ids.push_back(b);
    if (!ids.empty()) want.push_back({e, ids});
  }
  const auto without = ragged_classes(n, k, stripes, pres.data(), false);
  CHECK(without.size() == want.size());
  for (size_t c = 0; c < want.size(); ++c)
    CHECK(without[c].rows == want[c].first && without[c].stripes == want[c].second);

  std::vector<int> order(stripes);
  for (int b = 0; b < stripes; ++b) order[b] = b;
  std::shuffle(order.begin(), order.end(), rng);
  const size_t per = pattern_arena_bytes(k, m);
  for (size_t budget : {size_t(1), per, 2 * per, 5 * per + 7, 1000 * per}) {
    const size_t cap = std::max<size_t>(1, budget / per);
    std::vector<std::pair<size_t, size_t>> cuts;
    std::vector<std::vector<uint8_t>> held;
    size_t begin = 0;
    for (size_t j = 0; j < order.size(); ++j) {
      const std::vector<uint8_t> mask(pres.begin() + order[j] * n, pres.begin() + (order[j] + 1) * n);
      const bool known = std::find(held.begin(), held.end(), mask) != held.end();
      if (!known && held.size() == cap) {
        cuts.push_back({begin, j});
        begin = j;
        held.clear();
      }
      if (!known) held.push_back(mask);
    }
    cuts.push_back({begin, order.size()});
    CHECK(ragged_segments(k, n, m, order, pres.data(), budget) == cuts);
  }
}

// The form the update and locate routes call: a flag row of any width and the caller's own cost
// per pattern. The expectation is written out from the rule (a segment ends before the row that
// would be one distinct row more than max(1, budget / per)); the class form is this one at
// width n and pattern_arena_bytes.
void check_segments_of_any_row(int k, int m, std::mt19937& rng) {
  const int n = k + m, stripes = 50;
  for (const size_t width : {size_t(1), static_cast<size_t>(k), static_cast<size_t>(n)}) {
    std::vector<uint8_t> rows(static_cast<size_t>(stripes) * width);
    for (uint8_t& f : rows) f = static_cast<uint8_t>(rng() % 2);
    for (int b = 5; b < stripes; b += 2) {  // repeats of earlier rows
      const size_t src = rng() % static_cast<unsigned>(b);
      std::copy(rows.begin() + src * width, rows.begin() + (src + 1) * width, rows.begin() + b * width);
    }
    std::vector<int> order(stripes);
    for (int b = 0; b < stripes; ++b) order[b] = b;
    std::shuffle(order.begin(), order.end(), rng);
    order.resize(40);  // a call's runnable stripes: not every row is named
    for (const size_t per : {size_t(0), size_t(1), size_t(1000), pattern_arena_bytes(k, m) + 77})
      for (const size_t budget : {size_t(0), size_t(999), size_t(1000), size_t(3500), size_t(1) << 30}) {
        const size_t cap = std::max<size_t>(1, budget / std::max<size_t>(per, 1));
        std::vector<std::pair<size_t, size_t>> cuts;
        std::vector<std::vector<uint8_t>> held;
        size_t begin = 0;
        for (size_t j = 0; j < order.size(); ++j) {
          const std::vector<uint8_t> row(rows.begin() + order[j] * width, rows.begin() + (order[j] + 1) * width);
          const bool known = std::find(held.begin(), held.end(), row) != held.end();
          if (!known && held.size() == cap) {
            cuts.push_back({begin, j});
            begin = j;
            held.clear();
          }
          if (!known) held.push_back(row);
        }
        cuts.push_back({begin, order.size()});
        CHECK(ragged_segments(width, per, order, rows.data(), budget) == cuts);
        if (width == static_cast<size_t>(n) && per == pattern_arena_bytes(k, m) + 77)
          CHECK(ragged_segments(k, n, m, order, rows.data(), budget) ==
                ragged_segments(width, pattern_arena_bytes(k, m), order, rows.data(), budget));
      }
    CHECK(ragged_segments(width, 1000, {}, rows.data(), 1000).empty());
  }
}

// A run's set-up: the shape from the per-stripe rows, and the work list's items and chunks.
void check_shape_and_work(int k, int m) {
  struct G {
    int R;
  };
  const std::vector<G> groups = {{16}, {3}};
  const std::vector<size_t> sizes = {100003, 17, 8197, 40003, 9, 65536};
  const RaggedShape sh = ragged_shape(k, groups, sizes, [&](int s) { return std::make_pair(k + s % 2, m - s % 2); });
  CHECK(sh.k == k && sh.group_rows == std::vector<int>({16, 3}) && sh.size == sizes);
  for (int s = 0; s < sh.stripes(); ++s) CHECK(sh.nin[s] == k + s % 2 && sh.nout[s] == m - s % 2);
  const size_t budget = 64u << 10;
  RaggedWork w(sh, budget);
  CHECK(w.chunks.empty() && w.items.size() == ragged_items(sh, budget).size());
  CHECK(w.cut(sh, budget));
  const auto want = ragged_chunks(sh, w.items, budget);
  CHECK(w.chunks.size() == want.size() && w.chunks.size() > 3);
  for (size_t c = 0; c < want.size(); ++c)
    CHECK(w.chunks[c].first == want[c].first && w.chunks[c].count == want[c].count &&
          w.chunks[c].out_end == want[c].out_end && w.chunks[c].ntiles == want[c].ntiles);
  // the tile-map part of the metadata is fill_chunk_meta's
  for (const ChunkLayout& C : w.chunks) {
    std::vector<uint8_t> h(C.out_end, 0xEE);
    fill_chunk_tile_map(C, w.items, h.data());
    const auto* size = reinterpret_cast<const uint64_t*>(h.data() + C.size_off);
    const auto* tile0 = reinterpret_cast<const uint32_t*>(h.data() + C.tile0_off);
    const auto* tile_stripe = reinterpret_cast<const uint32_t*>(h.data() + C.tile_stripe_off);
    uint32_t t = 0;
    for (size_t j = 0; j < C.count; ++j) {
      CHECK(size[j] == w.items[C.first + j].w && tile0[j] == t);
      for (uint64_t q = 0; q < ragged_tiles(w.items[C.first + j].w); ++q) CHECK(tile_stripe[t++] == j);
    }
    CHECK(tile0[C.count] == t && t == C.ntiles);
    CHECK(h[C.in_tab_off] == 0xEE && h[C.pat_off] == 0xEE && h[C.status_off] == 0xEE);
  }
}

}  // namespace

int main() {
  std::mt19937 rng(0xC4A6);
  const std::vector<size_t> edge = {1, 15, 16, 17, 8191, 8192, 8193, 3 * 8192 + 83, 100003};
  for (const auto& km : {std::pair<int, int>{4, 2}, std::pair<int, int>{20, 10}}) {
    const int k = km.first, m = km.second;
    for (size_t budget : {size_t(64) << 10, size_t(16) << 20}) {
      std::vector<std::vector<size_t>> lists = {edge};
      for (int t = 0; t < 3; ++t) {
        std::vector<size_t> s(edge);
        for (int j = 0; j < 20; ++j) s.push_back(1 + rng() % (t == 0 ? 300 : t == 1 ? 20000 : 300000));
        std::shuffle(s.begin(), s.end(), rng);
        lists.push_back(s);
      }
      for (const auto& sizes : lists) {
        const int stripes = static_cast<int>(sizes.size());
        // with compares (encode / verify != 0): m rows per pattern
        check_run(k, m, m, false, sizes, random_masks(k, m, stripes, rng, 0), budget);
        // verify == 0 classes: exactly e missing
        for (int e : {1, m}) {
          std::vector<uint8_t> pres(static_cast<size_t>(stripes) * (k + m), 1);
          for (int b = 0; b < stripes; ++b)
            for (int j = 0; j < e; ++j) pres[static_cast<size_t>(b) * (k + m) + (b + j) % (k + m)] = 0;
          check_run(k, m, e, true, sizes, pres, budget);
        }
      }
    }
    check_classes_and_segments(k, m, rng);
    check_all_wanted_rules(k, m, rng);
    check_segments_of_any_row(k, m, rng);
    check_shape_and_work(k, m);
  }
  // an RS(128,128) batch of 500 patterns stays within the arena budget per segment
  {
    const int k = 128, m = 128, n = 256, stripes = 500;
    std::vector<uint8_t> pres(static_cast<size_t>(stripes) * n, 1);
    std::vector<int> all(stripes);
    for (int b = 0; b < stripes; ++b) {
      all[b] = b;
      pres[static_cast<size_t>(b) * n + b % n] = 0;
      pres[static_cast<size_t>(b) * n + (b / n + b + 1) % n] = 0;
    }
    const size_t per = pattern_arena_bytes(k, m);
    CHECK(per == 8u * 128 * 32 * 16);
    const auto segs = ragged_segments(k, n, m, all, pres.data(), kRaggedArenaBudget);
    CHECK(segs.size() >= 500 * per / kRaggedArenaBudget);
    for (const auto& s : segs) CHECK((s.second - s.first) * per <= kRaggedArenaBudget);
  }
  std::printf("ragged_chunks_test ok\n");
  return 0;
}
