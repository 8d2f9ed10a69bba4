// The message table of a checksummed codec batch (rs_codec_encode_batch_sums /
// rs_codec_decode_batch_sums): which rows of which item of a chunk are hashed,
// the result slot of each and the (stripe, shard) it stands for, the table sha256_rows
// (sha256.hpp) reads in descending order of length, and the one rule that says whether a
// chunk's shards hash on the device or on the host. Plain C++ with no HIP dependence:
// tests/native/sums_table_test.cpp builds it with g++ on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ragged_chunks.hpp"

namespace callfs {

// CALLFS_RS_SUMS_DEVICE: auto (the rule below), 0 (host always), 1 (the device for every
// whole-stripe item).
enum class SumsKnob { kAuto, kHost, kDevice };

// `auto`: a chunk hashes on the device when it holds at least kSumsAutoMinCount messages and
// its longest message has at most kSumsAutoMaxLen bytes. A lane hashes about 25 MB/s whatever
// its wave's other lanes do, so a chunk's hash launch lasts as long as its longest message,
// while the copy pool's time follows the chunk's bytes: the device is ahead where a chunk
// holds many short messages. Fitted to tools/jobs.sh sums_bench (profiles/r08/sums/sums.jsonl,
// DESIGN.md §7.7; 16 MiB chunks): with 16 KiB shards (853 and 956 messages per chunk) the
// device route took 0.60-0.69 of the host route's time, with 64 KiB shards (213 and 240
// messages) 1.10-2.01 of it. The constants are the last point at which the sweep has the device
// ahead; between them and the next point nothing is measured.
constexpr size_t kSumsAutoMinCount = 800;
constexpr size_t kSumsAutoMaxLen = 16384;

// What the table's dwords can say: a length below 4 GiB, an offset / 16 below 2^32.
constexpr uint64_t kSumsMaxChunk = 1ull << 36;

// The rule. count: the chunk's messages; longest: its longest message in bytes.
inline bool sums_on_device(SumsKnob knob, size_t count, size_t longest) {
  if (count == 0 || longest > 0xFFFFFFFFull || knob == SumsKnob::kHost) return false;
  if (knob == SumsKnob::kDevice) return true;
  return count >= kSumsAutoMinCount && longest <= kSumsAutoMaxLen;
}

// One result slot of a chunk: the run's stripe and the shard whose bytes the row holds, where
// the row lies in the chunk and how long the message is (the item's width, not its pitch).
struct SumsSlot {
  int stripe = 0;
  int shard = 0;
  size_t off = 0;
  size_t len = 0;
};

// The slots of chunk C in slot order: per whole-stripe item its staged rows (the pattern's
// valid[], then its compared rows), then -- digest mode -- its written rows (rows[0, missing)).
inline std::vector<SumsSlot> sums_slots(const ChunkLayout& C, const RaggedShape& sh,
                                        const std::vector<RaggedItem>& items, const MixedTables& mt) {
  std::vector<SumsSlot> slots;
  if (C.sums == SumsMode::kNone) return slots;
  slots.reserve(C.sums_count);
  const size_t k = static_cast<size_t>(sh.k);
  for (size_t j = 0; j < C.count; ++j) {
    const RaggedItem& it = items[C.first + j];
    const size_t rows = sums_rows(sh, it, C.sums);
    if (!rows) continue;
    const MixedPattern& pt = mt.patterns[mt.pat[static_cast<size_t>(it.stripe)]];
    const ItemLayout& il = C.items[j];
    const size_t nin = static_cast<size_t>(sh.nin[static_cast<size_t>(it.stripe)]);
    for (size_t r = 0; r < rows; ++r) {
      SumsSlot s;
      s.stripe = it.stripe;
      s.len = it.w;
      if (r < nin) {
        s.shard = r < k ? pt.valid[r] : pt.rows[static_cast<size_t>(pt.missing) + (r - k)];
        s.off = il.in_off + il.pitch * r;
      } else {
        s.shard = pt.rows[r - nin];
        s.off = il.out_off + il.pitch * (r - nin);
      }
      slots.push_back(s);
    }
  }
  return slots;
}

// The table at `tab` ([slots][3] dwords {offset / 16, length, slot}) in descending order of
// length, slots of one length in slot order: neighbouring lanes get messages of equal or
// near-equal length, so a wave does not wait on one long message.
inline void sums_fill_table(const std::vector<SumsSlot>& slots, uint32_t* tab) {
  std::vector<uint32_t> order(slots.size());
  for (size_t s = 0; s < slots.size(); ++s) order[s] = static_cast<uint32_t>(s);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return slots[a].len > slots[b].len; });
  for (size_t e = 0; e < order.size(); ++e) {
    const SumsSlot& s = slots[order[e]];
    tab[3 * e + 0] = static_cast<uint32_t>(s.off / 16);
    tab[3 * e + 1] = static_cast<uint32_t>(s.len);
    tab[3 * e + 2] = order[e];
  }
}

// Applies the rule to every chunk of a run packed with the sums regions (ragged_chunks with
// `mode`): a chunk the rule sends to the host is laid out again without them (the same items:
// it only shrinks). Returns a flag per stripe of the run: 1 where the stripe's shards hash on
// the host -- every stripe cut into column parts, and every whole-stripe item of a chunk
// that does not hash on the device.
inline std::vector<uint8_t> sums_route(const RaggedShape& sh, const std::vector<RaggedItem>& items,
                                       std::vector<ChunkLayout>& chunks, SumsKnob knob) {
  std::vector<uint8_t> host(static_cast<size_t>(sh.stripes()), 1);
  for (ChunkLayout& C : chunks) {
    if (C.sums == SumsMode::kNone) continue;
    size_t longest = 0;
    for (size_t j = 0; j < C.count; ++j)
      if (whole_stripe(sh, items[C.first + j])) longest = std::max(longest, items[C.first + j].w);
    if (!sums_on_device(knob, C.sums_count, longest) || C.out_end >= kSumsMaxChunk) {
      C = layout_chunk(sh, items, C.first, C.count, true, SumsMode::kNone);
      continue;
    }
    for (size_t j = 0; j < C.count; ++j)
      if (whole_stripe(sh, items[C.first + j])) host[static_cast<size_t>(items[C.first + j].stripe)] = 0;
  }
  return host;
}

}  // namespace callfs
