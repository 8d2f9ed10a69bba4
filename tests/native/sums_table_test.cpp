// The message table of the checksummed codec batches (callfs_amd/csrc/sums_table.hpp) and the
// optional regions of the chunk layout (ragged_chunks.hpp) on the CPU, built with g++
// -fsanitize=address,undefined by tests/test_native_sums.py. Over seeded runs of RS(4,2),
// RS(10,4) and RS(3,18) (two launch groups) at budgets of 64 KiB and 16 MiB, encodes (digest
// mode) and decodes with random erasures (check mode):
//  - without the regions the layout is byte for byte what it was (every offset of
//    layout_chunk(..., kNone) equals the five-argument call's), and a layout with them differs
//    only by the three regions, which lie inside the metadata, behind the input rows and behind
//    the status words, 256-B aligned and disjoint from every row;
//  - the slots of a chunk are exactly the hashed rows of its whole-stripe items: an encode's
//    k + m shards, a decode's present shards; each (stripe, shard) occurs once, its offset is
//    the row's and its length the item's width, never its pitch; column parts have no slot;
//  - the table is a permutation of the slots in descending order of length with offsets / 16;
//  - the rule: knob 0 sends every stripe to the host, knob 1 every whole-stripe item to the
//    device and every column part to the host, auto follows the two constants; a chunk sent to
//    the host is laid out as if the regions had never been asked for.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "gf256.hpp"
#include "mixed_tables.hpp"
#include "sums_table.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

void same_layout(const ChunkLayout& a, const ChunkLayout& b) {
  CHECK(a.first == b.first && a.count == b.count && a.in_tab_off == b.in_tab_off);
  CHECK(a.pat_off == b.pat_off && a.size_off == b.size_off && a.tile0_off == b.tile0_off);
  CHECK(a.tile_stripe_off == b.tile_stripe_off && a.item_tab_off == b.item_tab_off);
  CHECK(a.out_tab_off == b.out_tab_off && a.meta_end == b.meta_end && a.in_end == b.in_end);
  CHECK(a.status_off == b.status_off && a.out_end == b.out_end && a.ntiles == b.ntiles);
  for (size_t j = 0; j < a.count; ++j)
    CHECK(a.items[j].in_off == b.items[j].in_off && a.items[j].out_off == b.items[j].out_off &&
          a.items[j].pitch == b.items[j].pitch);
}

void check_run(int k, int m, bool decode, const std::vector<size_t>& sizes, std::mt19937& rng, size_t budget) {
  const int n = k + m, stripes = static_cast<int>(sizes.size());
  std::vector<uint8_t> pres(static_cast<size_t>(stripes) * n, 1);
  for (int b = 0; b < stripes; ++b) {
    if (!decode) {
      for (int i = k; i < n; ++i) pres[static_cast<size_t>(b) * n + i] = 0;
      continue;
    }
    // a decode class: every stripe has m rows (missing + compared), any erasure count 0..m
    const int e = static_cast<int>(rng() % static_cast<unsigned>(m + 1));
    for (int j = 0; j < e;) {
      const int i = static_cast<int>(rng() % static_cast<unsigned>(n));
      if (pres[static_cast<size_t>(b) * n + i]) {
        pres[static_cast<size_t>(b) * n + i] = 0;
        ++j;
      }
    }
  }
  MixedTables mt;
  CHECK(build_mixed_tables(k, m, stripes, pres.data(), nullptr, mt, decode) == TableError::kOk);
  RaggedShape sh;
  sh.k = k;
  for (const MixedGroup& g : mt.groups) sh.group_rows.push_back(g.R);
  for (int b = 0; b < stripes; ++b) {
    const MixedPattern& pt = mt.patterns[mt.pat[b]];
    sh.size.push_back(sizes[b]);
    sh.nin.push_back(k + static_cast<int>(pt.rows.size()) - pt.missing);
    sh.nout.push_back(pt.missing);
  }
  const SumsMode mode = decode ? SumsMode::kCheck : SumsMode::kDigest;
  const std::vector<RaggedItem> items = ragged_items(sh, budget);
  const std::vector<ChunkLayout> plain = ragged_chunks(sh, items, budget);
  for (const ChunkLayout& C : plain) {
    same_layout(C, layout_chunk(sh, items, C.first, C.count, true, SumsMode::kNone));
    CHECK(C.sums == SumsMode::kNone && C.sums_count == 0);
    CHECK(sums_slots(C, sh, items, mt).empty());
  }

  for (SumsKnob knob : {SumsKnob::kHost, SumsKnob::kDevice, SumsKnob::kAuto}) {
    std::vector<ChunkLayout> chunks =
        ragged_chunks(sh, items, budget, true, knob == SumsKnob::kHost ? SumsMode::kNone : mode);
    const std::vector<uint8_t> host = sums_route(sh, items, chunks, knob);
    CHECK(host.size() == static_cast<size_t>(stripes));
    std::set<std::pair<int, int>> seen;
    size_t next = 0;
    for (const ChunkLayout& C : chunks) {
      CHECK(C.first == next);
      next += C.count;
      const ChunkLayout bare = layout_chunk(sh, items, C.first, C.count);
      size_t want = 0, longest = 0;
      for (size_t j = 0; j < C.count; ++j) {
        const RaggedItem& it = items[C.first + j];
        if (!whole_stripe(sh, it)) {
          CHECK(host[static_cast<size_t>(it.stripe)] == 1);  // column parts: always the host
          continue;
        }
        want += static_cast<size_t>(sh.nin[it.stripe]) + (decode ? 0 : static_cast<size_t>(sh.nout[it.stripe]));
        longest = std::max(longest, it.w);
      }
      const bool dev = sums_on_device(knob, want, longest);
      if (knob == SumsKnob::kHost) CHECK(!dev);
      if (knob == SumsKnob::kDevice) CHECK(dev == (want > 0));
      if (knob == SumsKnob::kAuto) CHECK(dev == (want >= kSumsAutoMinCount && longest <= kSumsAutoMaxLen));
      if (!dev) {
        same_layout(C, bare);
        CHECK(C.sums_count == 0 && C.sums == SumsMode::kNone);
        for (size_t j = 0; j < C.count; ++j) CHECK(host[static_cast<size_t>(items[C.first + j].stripe)] == 1);
        continue;
      }
      CHECK(C.sums == mode && C.sums_count == want);
      // the regions: in the metadata, behind the input rows, behind the status words
      CHECK(C.sums_tab_off % 256 == 0 && C.sums_tab_off >= C.item_tab_off + 16 * C.count);
      CHECK(C.sums_tab_off + 12 * want <= C.meta_end);
      CHECK(C.sums_out_off % 256 == 0 && C.sums_out_off >= C.status_off + sizeof(int) * C.count);
      const size_t out_bytes = (decode ? 1 : 32) * want;
      if (decode) {
        CHECK(C.sums_expect_off % 256 == 0 && C.sums_expect_off + 32 * want <= C.in_end);
      }
      for (size_t j = 0; j < C.count; ++j) {
        const RaggedItem& it = items[C.first + j];
        const ItemLayout& il = C.items[j];
        CHECK(il.in_off >= C.meta_end && il.pitch == round_up(it.w, 16));
        CHECK(il.in_off + il.pitch * static_cast<size_t>(sh.nin[it.stripe]) <=
              (decode ? C.sums_expect_off : C.in_end));
        if (sh.nout[it.stripe]) CHECK(il.out_off >= C.sums_out_off + out_bytes);
        CHECK(il.out_off + il.pitch * static_cast<size_t>(sh.nout[it.stripe]) <= C.out_end);
      }
      // the slots
      const std::vector<SumsSlot> slots = sums_slots(C, sh, items, mt);
      CHECK(slots.size() == want);
      for (size_t j = 0; j < C.count; ++j) {
        const RaggedItem& it = items[C.first + j];
        if (!whole_stripe(sh, it)) continue;
        CHECK(host[static_cast<size_t>(it.stripe)] == 0);
        const MixedPattern& pt = mt.patterns[mt.pat[it.stripe]];
        const size_t s0 = C.sums_slot0[j];
        const size_t nin = static_cast<size_t>(sh.nin[it.stripe]);
        std::set<int> shards;
        const size_t rows = nin + (decode ? 0 : static_cast<size_t>(sh.nout[it.stripe]));
        for (size_t r = 0; r < rows; ++r) {
          const SumsSlot& s = slots[s0 + r];
          CHECK(s.stripe == it.stripe && s.len == it.w && s.off % 16 == 0);
          CHECK(pres[static_cast<size_t>(it.stripe) * n + s.shard] == (r < nin ? 1 : 0));
          if (r < static_cast<size_t>(k)) CHECK(s.shard == pt.valid[r]);
          CHECK(s.off == (r < nin ? C.items[j].in_off + C.items[j].pitch * r
                                  : C.items[j].out_off + C.items[j].pitch * (r - nin)));
          CHECK(shards.insert(s.shard).second);
          CHECK(seen.insert({it.stripe, s.shard}).second);
        }
        // an encode hashes all n shards, a decode every present one
        int np = 0;
        for (int i = 0; i < n; ++i) np += pres[static_cast<size_t>(it.stripe) * n + i];
        CHECK(shards.size() == static_cast<size_t>(decode ? np : n));
      }
      // the table
      std::vector<uint32_t> tab(3 * want + 1, 0xDEADBEEFu);
      sums_fill_table(slots, tab.data());
      CHECK(tab[3 * want] == 0xDEADBEEFu);
      std::set<uint32_t> used;
      for (size_t e = 0; e < want; ++e) {
        const uint32_t slot = tab[3 * e + 2];
        CHECK(slot < want && used.insert(slot).second);
        CHECK(static_cast<size_t>(tab[3 * e]) * 16 == slots[slot].off && tab[3 * e + 1] == slots[slot].len);
        if (e) CHECK(tab[3 * e + 1] <= tab[3 * (e - 1) + 1]);
        if (e && tab[3 * e + 1] == tab[3 * (e - 1) + 1]) CHECK(slot > tab[3 * (e - 1) + 2]);
      }
    }
    CHECK(next == items.size());
    // every stripe is hashed on exactly one side
    for (int b = 0; b < stripes; ++b)
      if (!host[static_cast<size_t>(b)]) CHECK(seen.count({b, mt.patterns[mt.pat[b]].valid[0]}) == 1);
  }
}

}  // namespace

int main() {
  CHECK(!sums_on_device(SumsKnob::kHost, 100000, 256));
  CHECK(sums_on_device(SumsKnob::kDevice, 1, 1u << 20));
  CHECK(!sums_on_device(SumsKnob::kDevice, 0, 0));
  CHECK(!sums_on_device(SumsKnob::kDevice, 4, 1ull << 32));  // the table's length is a dword
  CHECK(sums_on_device(SumsKnob::kAuto, kSumsAutoMinCount, kSumsAutoMaxLen));
  CHECK(!sums_on_device(SumsKnob::kAuto, kSumsAutoMinCount - 1, kSumsAutoMaxLen));
  CHECK(!sums_on_device(SumsKnob::kAuto, kSumsAutoMinCount, kSumsAutoMaxLen + 1));
  std::mt19937 rng(20261020);
  const int profiles[][2] = {{4, 2}, {10, 4}, {3, 18}};
  for (const auto& p : profiles)
    for (size_t budget : {size_t(64) << 10, size_t(16) << 20})
      for (int decode = 0; decode < 2; ++decode)
        for (int round = 0; round < 4; ++round) {
          std::vector<size_t> sizes;
          const int stripes = 1 + static_cast<int>(rng() % 300);
          for (int b = 0; b < stripes; ++b) {
            const unsigned pick = rng() % 16;
            sizes.push_back(pick == 0 ? 1 + rng() % 400000   // cut into column parts at 64 KiB
                            : pick < 4 ? 1 + rng() % 20       // shorter than one vector
                                       : 1 + rng() % 5000);
          }
          check_run(p[0], p[1], decode != 0, sizes, rng, budget);
        }
  // a run large enough for `auto` to pick the device
  {
    std::vector<size_t> sizes(400, 256);
    check_run(10, 4, false, sizes, rng, size_t(16) << 20);
    check_run(10, 4, true, sizes, rng, size_t(16) << 20);
  }
  std::printf("sums_table_test ok\n");
  return 0;
}
