// Correct on host memory: rs_correct, rs_correct_batch and the correction
// step of rs_codec_decode_correct are the locate route of host_locate.hpp with launch_correct
// in launch_locate's place. A chunk's counts come back first; then only the (item, shard) rows
// whose count is nonzero -- the rows the launch changed -- are copied from the slot's device
// mirror into the caller's shards, one D2H each. A chunk of clean stripes copies no shard byte
// back. Included by rs_host.cpp only.
#pragma once

#include "host_locate.hpp"

namespace callfs {
namespace {

// After a chunk: input row i of an item is its pattern's valid[i], row k + x its compared shard
// x (as staged by run_locate_chunks). shards: the call's, batch * (k + m).
struct CorrectBack {
  uint8_t* const* shards;
  int operator()(const LocateRun& r, const ChunkLayout& C, const std::vector<RaggedItem>& items,
                 const uint8_t* d, const uint64_t* cn) const {
    const size_t k = static_cast<size_t>(r.k), n = static_cast<size_t>(r.k + r.m), nb = r.bins();
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      const size_t id = static_cast<size_t>(r.ids[static_cast<size_t>(it.stripe)]);
      const uint32_t p = r.mt().pat[static_cast<size_t>(it.stripe)];
      const MixedPattern& pt = r.mt().patterns[p];
      const size_t rows = r.t.rows(p);
      for (size_t row = 0; row < k + rows; ++row) {
        const size_t shard = static_cast<size_t>(row < k ? pt.valid[row] : pt.rows[row - k]);
        if (cn[j * nb + shard] == 0) continue;
        HIPCHK(hipMemcpy(shards[id * n + shard] + it.off, d + il.in_off + il.pitch * row, it.w,
                         hipMemcpyDeviceToHost));
        r.ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
      }
    }
    return RS_OK;
  }
};

// Shared by rs_correct, rs_correct_batch and rs_codec_decode_correct: locate_batch_host's
// admission (a stripe of exactly k present shards is RS_OK with zero counts and no device
// work), then the correcting pipeline. counts: batch * (k + m + 1), written for every stripe:
// the bytes changed per shard, and the columns left mismatching. status[b] = RS_E_CORRUPT where
// a column of stripe b is left.
int correct_batch_host(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards, const size_t* lens,
                       uint64_t* counts, int* status) {
  const size_t n = static_cast<size_t>(k + m), B = static_cast<size_t>(batch);
  std::fill(counts, counts + B * (n + 1), 0);
  std::vector<uint8_t> present(B * n, 0), none(n, 0), row(n, 0);
  std::vector<size_t> S(B, 0);
  std::vector<int> ids;
  for (size_t b = 0; b < B; ++b) {
    const StripeAdmission a = admit_stripe(k + m, k, shards + b * n, lens + b * n, none.data(), true, row.data());
    status[b] = a.status;
    if (!a.run) continue;
    S[b] = a.S;
    for (size_t i = 0; i < n; ++i) present[b * n + i] = row[i] == kShardPresent;
    ids.push_back(static_cast<int>(b));
  }
  std::vector<int> flags(B, 0);
  const int rc = run_locate(ctx, k, m, 1, ids, S.data(), present.data(),
                            [&](int b, int i) { return shards[static_cast<size_t>(b) * n + i]; }, counts,
                            flags.data(), /*correct=*/true, CorrectBack{shards});
  if (rc) return rc;
  for (size_t b = 0; b < B; ++b)
    if (counts[b * (n + 1) + n] != 0) status[b] = RS_E_CORRUPT;
  return RS_OK;
}

}  // namespace
}  // namespace callfs
