// The per-object plan of the codec-level batch calls (rs_codec_encode_batch /
// rs_codec_decode_batch): upstream Split's shape of one object (shard size,
// full shards, zero pad), where each input row of its encode is read from, and the Join
// (host_path.hpp) through which the pipeline's staging copies tee an encode's full data
// shards into shards_out and a decode's data shards into the joined object. Plain C++ with
// no HIP dependence: tests/native/codec_batch_test.cpp checks it with g++ on the CPU;
// rs_host.cpp is the product user.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "host_path.hpp"

namespace callfs {

// Upstream Split of an object of len > 0 bytes into k data shards (codec.go:31).
struct SplitPlan {
  int k = 0;
  size_t len = 0;
  size_t S = 0;     // shard size: ceil(len / k)
  size_t full = 0;  // data shards that lie wholly inside the object: len / S
  size_t pad = 0;   // zero bytes behind the object: k * S - len
  // Rows [0, rows_from_data) are staged straight from the caller's `data`, the others from
  // shards_out: `full` when data and shards_out are disjoint, 0 when the object is split
  // in place.
  size_t rows_from_data = 0;
};

inline SplitPlan split_plan(int k, size_t len) {
  SplitPlan p;
  p.k = k;
  p.len = len;
  p.S = (len + static_cast<size_t>(k) - 1) / static_cast<size_t>(k);
  p.full = len / p.S;
  p.pad = p.S * static_cast<size_t>(k) - len;
  return p;
}

// Readies shards_out (n * S bytes) for the pipeline as rs_codec_encode does and sets
// p.rows_from_data. In place (shards_out == data) only the pad is zeroed; buffers that
// overlap partly are moved first and then count as in place; disjoint ones receive the
// partial last shard (and any shard that is all padding) and the pad, and the full shards
// stay in `data`.
inline void split_prepare(SplitPlan& p, int n, const uint8_t* data, uint8_t* shards_out) {
  const bool overlap = shards_out != data && shards_out < data + p.len &&
                       data < shards_out + p.S * static_cast<size_t>(n);
  if (shards_out == data || overlap) {
    if (overlap) std::memmove(shards_out, data, p.len);
    p.rows_from_data = 0;
  } else {
    std::memcpy(shards_out + p.full * p.S, data + p.full * p.S, p.len - p.full * p.S);
    p.rows_from_data = p.full;
  }
  std::memset(shards_out + p.len, 0, p.pad);
}

// Where the pipeline reads data shard i (i < k) of the object.
inline const uint8_t* split_row(const SplitPlan& p, const uint8_t* data, const uint8_t* shards_out,
                                int i) {
  const size_t at = p.S * static_cast<size_t>(i);
  return static_cast<size_t>(i) < p.rows_from_data ? data + at : shards_out + at;
}

// The tee of an encode: the rows staged from `data` also land in shards_out, bytes
// [0, rows_from_data * S). (join_span of a column part then gives that part's range.)
inline Join split_tee(const SplitPlan& p, uint8_t* shards_out) {
  return Join{shards_out, p.rows_from_data * p.S, p.S, p.k};
}

// The join of a decode (codec.go:67-77): out receives bytes [0, min(original_size, k * S))
// of the data shards laid end to end.
inline Join decode_join(int k, size_t S, uint8_t* out, size_t original_size) {
  return Join{out, std::min(original_size, S * static_cast<size_t>(k)), S, k};
}

}  // namespace callfs
