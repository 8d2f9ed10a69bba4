// The planner of rs_codec_overwrite: an object laid out as Split lays it
// (object byte x in data shard x / S at column x % S) has the byte range [offset, offset + len)
// overwritten. A column of the stripe sees the shards the range covers at that column: the
// range's first shard from its first column on, its last shard up to its last column, every
// shard between them everywhere. So [0, S) falls into at most three disjoint column intervals,
// cut at the first column of the first shard and behind the last column of the last shard, and
// the shards changed in an interval are consecutive. Each interval becomes one stripe of an
// rs_update_batch; disjoint columns are disjoint parity bytes, so the stripes never race.
// Plain C++ with no HIP dependence: tests/native/update_host_test.cpp checks it by brute force.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace callfs {

struct OverwriteInterval {
  size_t col0 = 0, col1 = 0;     // columns [col0, col1), never empty
  int shard0 = 0, shard1 = 0;    // changed data shards shard0 .. shard1 inclusive, never empty
};

// False when the range is empty or does not lie inside the k * S object bytes. The intervals
// come out in ascending column order, pairwise disjoint, covering exactly the columns the
// range touches.
inline bool overwrite_plan(int k, size_t S, uint64_t offset, uint64_t len,
                           std::vector<OverwriteInterval>& out) {
  out.clear();
  const uint64_t total = static_cast<uint64_t>(k) * S;
  if (len == 0 || S == 0 || offset >= total || len > total - offset) return false;
  const uint64_t last = offset + len - 1;
  const int a = static_cast<int>(offset / S), z = static_cast<int>(last / S);
  const size_t ca = static_cast<size_t>(offset % S);      // shard a changes at columns >= ca
  const size_t cz = static_cast<size_t>(last % S) + 1;    // shard z at columns < cz
  if (a == z) {
    out.push_back({ca, cz, a, a});
    return true;
  }
  const size_t cuts[4] = {0, std::min(ca, cz), std::max(ca, cz), S};
  for (int q = 0; q < 3; ++q) {
    const size_t lo = cuts[q], hi = cuts[q + 1];
    if (lo >= hi) continue;
    const int s0 = a + (lo < ca ? 1 : 0), s1 = z - (hi > cz ? 1 : 0);
    if (s0 > s1) continue;  // between the last shard's end and the first shard's start, no shard between
    out.push_back({lo, hi, s0, s1});
  }
  return true;
}

}  // namespace callfs
