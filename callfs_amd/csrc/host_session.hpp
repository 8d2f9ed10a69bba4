// The HIP-free parts of a decode session (rs_session_open): the environment
// knobs, which route a feed takes, and the book a session keeps of what was fed -- what a feed and
// a finish refuse, and the arrays of the final plan. Plain C++ with no HIP dependence;
// rs_session.cpp is the product user.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/callfs_rs.h"
#include "feed_tables.hpp"

namespace callfs {

// Source slots of a session's ring (CALLFS_RS_SESSION_SLOTS overrides, 1..8): a feed blocks only
// when every slot still holds a shard its launch has not finished with.
constexpr int kSessionMaxSlots = 8;
inline int session_slots() {
  static const int v = [] {
    const char* e = std::getenv("CALLFS_RS_SESSION_SLOTS");
    const int x = e ? std::atoi(e) : 3;
    return std::max(1, std::min(kSessionMaxSlots, x));
  }();
  return v;
}

// Shards of at most this many bytes are fed in place: the kernel reads the host-coherent slot
// over PCIe. Above it a feed is staged: one H2D into a device slot, then the launch.
// CALLFS_RS_SESSION_INPLACE_MAX overrides (0: every feed staged). The default is the value of
// CALLFS_RS_SMALL_MAX_BYTES' default, 2 MiB.
inline size_t session_inplace_max() {
  const char* e = std::getenv("CALLFS_RS_SESSION_INPLACE_MAX");
  return e ? static_cast<size_t>(std::strtoull(e, nullptr, 0)) : (2u << 20);
}

enum class FeedRoute { kDirect, kInPlace, kStaged };

// pinned: the shard lies inside an rs_host_alloc buffer, which the device reads where it is
inline FeedRoute feed_route(size_t S, size_t inplace_max, bool pinned) {
  if (S > inplace_max) return FeedRoute::kStaged;
  return pinned ? FeedRoute::kDirect : FeedRoute::kInPlace;
}

// What a session knows of its stripe and of the feeds so far.
struct SessionBook {
  int k = 0, n = 0;
  std::vector<uint8_t> expect, want, compare;  // n flags each
  std::vector<uint8_t> fed;                    // n flags
  int fed_expected = 0, feeds = 0;
  bool finished = false;

  void open(int k_, int n_, const uint8_t* e, const uint8_t* w, const uint8_t* c) {
    k = k_;
    n = n_;
    expect.assign(static_cast<size_t>(n), 0);
    want = compare = fed = expect;
    for (int i = 0; i < n; ++i) {
      expect[static_cast<size_t>(i)] = e[i] != 0;
      want[static_cast<size_t>(i)] = w[i] != 0;
      compare[static_cast<size_t>(i)] = c[i] != 0;
    }
  }
  // RS_OK when shard idx may be fed now: expected or compared, and not fed before
  int may_feed(int idx) const {
    if (finished || idx < 0 || idx >= n) return RS_E_ARG;
    const size_t i = static_cast<size_t>(idx);
    if (!(expect[i] || compare[i]) || fed[i]) return RS_E_ARG;
    return RS_OK;
  }
  void note_feed(int idx) {
    fed[static_cast<size_t>(idx)] = 1;
    fed_expected += expect[static_cast<size_t>(idx)];
    ++feeds;
  }
  bool has_row(int idx) const {
    return idx >= 0 && idx < n && (want[static_cast<size_t>(idx)] || compare[static_cast<size_t>(idx)]);
  }
  // RS_OK when the session may finish: every expected shard fed, and not finished before
  int may_finish() const {
    if (finished) return RS_E_ARG;
    return fed_expected < k ? RS_E_TOO_FEW_SHARDS : RS_OK;
  }
  // compared shards that arrived: the check rows of the final plan
  std::vector<int> delivered_compared() const {
    std::vector<int> v;
    for (int i = 0; i < n; ++i)
      if (compare[static_cast<size_t>(i)] && fed[static_cast<size_t>(i)]) v.push_back(i);
    return v;
  }
};

}  // namespace callfs
