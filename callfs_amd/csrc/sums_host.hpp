// The host side of the checksummed codec batches: what a call hands the
// ragged pipeline (SumsCall), the shards hashed by the copy pool's threads, one message per
// task (stripes cut into column parts, and whole stripes the rule of sums_table.hpp keeps off
// the device), and the bookkeeping of a decode's follow-up run over the objects that had a
// mismatch. Plain C++ with no HIP dependence: tests/native/sums_host_test.cpp drives it
// under ASan+UBSan against a software SHA-256.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "copy_pool.hpp"
#include "sha256_host.hpp"
#include "sums_table.hpp"

namespace callfs {

// A call's checksum arrays as the pipeline indexes them: shard i of runnable stripe `id` is
// entry obj[id] * n + i (of 32 bytes in digests / expected, of one byte in bad).
struct SumsCall {
  SumsMode mode = SumsMode::kNone;  // kDigest: an encode; kCheck: a decode
  int n = 0;
  const int* obj = nullptr;           // runnable stripe -> the call's object
  uint8_t* digests = nullptr;         // kDigest, written
  const uint8_t* expected = nullptr;  // kCheck, read
  uint8_t* bad = nullptr;             // kCheck, written: 1 = the shard's digest differs
  size_t at(int id, int shard) const {
    return static_cast<size_t>(obj[id]) * static_cast<size_t>(n) + static_cast<size_t>(shard);
  }
};

// One shard hashed on the host: its digest to `digest`, or compared with `expected` into *bad.
struct SumsTask {
  const uint8_t* msg = nullptr;
  size_t len = 0;
  uint8_t* digest = nullptr;
  const uint8_t* expected = nullptr;
  uint8_t* bad = nullptr;
};

inline SumsTask sums_task(const SumsCall& c, int id, int shard, const uint8_t* msg, size_t len) {
  const size_t at = c.at(id, shard);
  if (c.mode == SumsMode::kDigest) return {msg, len, c.digests + 32 * at, nullptr, nullptr};
  return {msg, len, nullptr, c.expected + 32 * at, c.bad + at};
}

inline void run_sums_tasks(CopyPool& pool, const std::vector<SumsTask>& tasks) {
  pool.each(tasks.size(), [&](size_t i) {
    const SumsTask& t = tasks[i];
    uint8_t d[32];
    sha256_host(t.msg, t.len, t.digest ? t.digest : d);
    if (t.expected) *t.bad = std::memcmp(d, t.expected, 32) != 0;
  });
}

// The follow-up run of a checked decode: the objects that ran (ran_S[b] != 0) and have a
// mismatch, as one batch for the plain decode path with the bad shards' lengths zero. The
// plain path then admits each of them again (RS_E_TOO_FEW_SHARDS where fewer than k good
// shards are left), rebuilds the bad shards into their own buffers beside the missing ones,
// verifies the rest and joins. finish() hands the outcome back: the status always, the
// lengths where the object ran (a refused object keeps the lengths it came with).
struct SumsRerun {
  std::vector<int> objs;  // the call's objects, ascending
  std::vector<uint8_t*> shards;
  std::vector<size_t> lens;
  std::vector<uint8_t*> out;
  std::vector<int64_t> sizes;
  std::vector<int> status;

  SumsRerun(int n, int batch, const size_t* ran_S, const uint8_t* bad, uint8_t* const* all_shards,
            const size_t* all_lens, uint8_t* const* all_out, const int64_t* all_sizes) {
    const size_t nn = static_cast<size_t>(n);
    for (int b = 0; b < batch; ++b) {
      const size_t at = static_cast<size_t>(b) * nn;
      bool any = false;
      for (size_t i = 0; ran_S[b] && i < nn; ++i) any |= bad[at + i] != 0;
      if (!any) continue;
      objs.push_back(b);
      for (size_t i = 0; i < nn; ++i) {
        shards.push_back(all_shards[at + i]);
        lens.push_back(bad[at + i] ? 0 : all_lens[at + i]);
      }
      out.push_back(all_out[b]);
      sizes.push_back(all_sizes[b]);
    }
    status.assign(objs.size(), 0);
  }
  int count() const { return static_cast<int>(objs.size()); }
  // ran(status): whether the plain path rebuilt the object's shards and set their lengths
  template <class Ran>
  void finish(int n, size_t* all_lens, int* all_status, Ran ran) const {
    const size_t nn = static_cast<size_t>(n);
    for (size_t j = 0; j < objs.size(); ++j) {
      const size_t b = static_cast<size_t>(objs[j]);
      all_status[b] = status[j];
      if (!ran(status[j])) continue;
      for (size_t i = 0; i < nn; ++i) all_lens[b * nn + i] = lens[j * nn + i];
    }
  }
};

}  // namespace callfs
