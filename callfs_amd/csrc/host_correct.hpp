// Correct on host memory: rs_correct, rs_correct_batch and the correction
// step of rs_codec_decode_correct are the locate route of host_locate.hpp as a correct run:
// launch_correct in launch_locate's place, and the rows a launch changed copied back into the
// caller's shards. Included by rs_host.cpp only.
#pragma once

#include "host_locate.hpp"

namespace callfs {
namespace {

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
                            flags.data(), /*repair=*/shards);
  if (rc) return rc;
  for (size_t b = 0; b < B; ++b)
    if (counts[b * (n + 1) + n] != 0) status[b] = RS_E_CORRUPT;
  return RS_OK;
}

}  // namespace
}  // namespace callfs
