// The HIP-free parts of an encode session (rs_encode_session_open): the slot
// size knob, how a feed is cut into slot-sized pieces, and the book a session keeps of the body
// ranges fed so far -- what a feed refuses and when the body is complete. The route of a piece is
// host_session.hpp's feed_route. Plain C++ with no HIP dependence; rs_encode_session.cpp is the
// product user, tests/native/absorb_tables_test.cpp checks it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

#include "host_session.hpp"

namespace callfs {

// Bytes of one source slot of an encode session's ring, and so the largest piece one launch
// takes (CALLFS_RS_ENCODE_SESSION_CHUNK overrides, at least 1; read at open).
inline size_t encode_session_chunk() {
  const char* e = std::getenv("CALLFS_RS_ENCODE_SESSION_CHUNK");
  const size_t v = e ? static_cast<size_t>(std::strtoull(e, nullptr, 0)) : (4u << 20);
  return std::max<size_t>(1, v);
}

// A session's slot: the whole body when it is smaller than the chunk.
inline size_t encode_session_slot(uint64_t L, size_t chunk) {
  return static_cast<size_t>(std::min<uint64_t>(L, chunk));
}

struct EncodePiece {
  uint64_t off;
  size_t n;
};

// [off, off + n) in consecutive pieces of at most `slot` bytes: one launch each.
inline void encode_pieces(uint64_t off, size_t n, size_t slot, std::vector<EncodePiece>& out) {
  out.clear();
  for (size_t at = 0; at < n; at += slot) out.push_back({off + at, std::min(slot, n - at)});
}

// What a session knows of its object and of the feeds so far: the fed ranges as a sorted set of
// disjoint intervals [first, second), neighbours merged.
struct EncodeBook {
  uint64_t L = 0;
  int k = 0;
  size_t S = 0;
  std::vector<std::pair<uint64_t, uint64_t>> fed;
  bool finished = false;

  void open(int k_, uint64_t L_) {
    k = k_;
    L = L_;
    S = static_cast<size_t>((L_ + static_cast<uint64_t>(k_) - 1) / static_cast<uint64_t>(k_));
    fed.clear();
    finished = false;
  }
  // RS_OK when [off, off + n) may be fed now: not empty, inside [0, L), disjoint from every fed
  // range, and not after a finish
  int may_feed(uint64_t off, uint64_t n) const {
    if (finished || n == 0 || off >= L || n > L - off) return RS_E_ARG;
    // the first interval that ends behind off
    auto it = std::upper_bound(fed.begin(), fed.end(), off,
                               [](uint64_t x, const std::pair<uint64_t, uint64_t>& r) { return x < r.second; });
    if (it != fed.end() && it->first < off + n) return RS_E_ARG;
    return RS_OK;
  }
  // after may_feed said RS_OK
  void note_feed(uint64_t off, uint64_t n) {
    auto it = std::upper_bound(fed.begin(), fed.end(), off,
                               [](uint64_t x, const std::pair<uint64_t, uint64_t>& r) { return x < r.second; });
    it = fed.insert(it, {off, off + n});
    if (it + 1 != fed.end() && (it + 1)->first == it->second) {
      it->second = (it + 1)->second;
      it = fed.erase(it + 1) - 1;
    }
    if (it != fed.begin() && (it - 1)->second == it->first) {
      (it - 1)->second = it->second;
      fed.erase(it);
    }
  }
  // exactly [0, L) is fed
  bool complete() const { return fed.size() == 1 && fed[0].first == 0 && fed[0].second == L; }
  uint64_t fed_bytes() const {
    uint64_t t = 0;
    for (const auto& r : fed) t += r.second - r.first;
    return t;
  }
};

}  // namespace callfs
