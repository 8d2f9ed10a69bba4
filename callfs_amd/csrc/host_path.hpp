// The HIP-free parts of the host-memory path and of the plans' buffer layout: the registry
// and pool of rs_host_alloc buffers, the chunk geometry of the pipeline, the join / tee
// targets, the argument checks and the admission of a reconstruct stripe (with or without a
// wanted set: one function, one flag encoding per shard), the stripe grouping and the routing
// of the batch calls, and the 256-byte packer of device buffers. Plain C++
// with no HIP dependence, so tests/native/host_test.cpp checks it on the CPU under ASan+UBSan
// and TSan; rs_context.cpp, rs_host.cpp (with its host_*.hpp) and rs_plan.cpp are the product
// users.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/callfs_rs.h"

namespace callfs {

constexpr size_t kPitchAlign = 256;

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Lays pieces out one after another, each starting on a 256-byte boundary: take(bytes)
// returns the piece's offset, `off` is the total so far (itself a multiple of 256).
struct Packer {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off = round_up(off + bytes, 256);
    return o;
  }
};

// Allocations made by rs_host_alloc: [base, base+size) ranges the host path may DMA
// from / to directly.
class PinnedRegistry {
 public:
  void add(void* p, size_t n) {
    std::lock_guard<std::mutex> g(mu_);
    ranges_[reinterpret_cast<uintptr_t>(p)] = n;
  }
  bool remove(void* p) {
    std::lock_guard<std::mutex> g(mu_);
    return ranges_.erase(reinterpret_cast<uintptr_t>(p)) == 1;
  }
  // size of the allocation starting at p (0 when p is not one)
  size_t size_of(void* p) const {
    std::lock_guard<std::mutex> g(mu_);
    auto it = ranges_.find(reinterpret_cast<uintptr_t>(p));
    return it == ranges_.end() ? 0 : it->second;
  }
  // true when [p, p+n) lies inside one registered allocation
  bool contains(const void* p, size_t n) const {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> g(mu_);
    auto it = ranges_.upper_bound(a);
    if (it == ranges_.begin()) return false;
    --it;
    return a >= it->first && a + n <= it->first + it->second;
  }
  bool empty() const {
    std::lock_guard<std::mutex> g(mu_);
    return ranges_.empty();
  }
  std::vector<void*> all() const {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<void*> v;
    for (const auto& r : ranges_) v.push_back(reinterpret_cast<void*>(r.first));
    return v;
  }

 private:
  mutable std::mutex mu_;
  std::map<uintptr_t, size_t> ranges_;
};

// Idle rs_host_alloc buffers kept for reuse. Page-locking a fresh buffer costs about
// 0.2 s per 384 MiB, so a server that allocates a pinned body per request and frees it
// after the call ran 25-30x slower than one that reuses buffers (RS(4,2) 256 MiB,
// zero-copy: 1.6 vs 48 GiB/s encode). rs_host_free parks a buffer here;
// rs_host_alloc takes the smallest parked buffer that fits without wasting more than a
// quarter of it, both sides counted in 2 MiB granules. Parked bytes are capped by `limit`
// (the context passes CALLFS_RS_HOST_POOL_BYTES, default 4 GiB; 0 disables parking):
// beyond it the largest parked buffers are released.
class HostPool {
 public:
  struct Buf {
    void* p;
    size_t cap;
  };
  explicit HostPool(size_t limit) : limit_(limit) {}
  // a parked buffer of at least n bytes, or {nullptr, 0}
  Buf take(size_t n) {
    // compare in allocation granules: a 4 KiB or 1 MiB request was allocated as one
    // 2 MiB granule, and that buffer must serve the next request of the same size
    const size_t want = granule(n);
    std::lock_guard<std::mutex> g(mu_);
    auto it = idle_.lower_bound(want);
    if (it == idle_.end() || it->first - want > it->first / 4) return {nullptr, 0};
    Buf b{it->second, it->first};
    idle_bytes_ -= it->first;
    idle_.erase(it);
    return b;
  }
  // park a buffer; returns the buffers to release now (over the cap)
  std::vector<void*> put(void* p, size_t cap) {
    std::vector<void*> drop;
    std::lock_guard<std::mutex> g(mu_);
    if (cap > limit_) {
      drop.push_back(p);
      return drop;
    }
    idle_.emplace(cap, p);
    idle_bytes_ += cap;
    while (idle_bytes_ > limit_ && !idle_.empty()) {
      auto last = std::prev(idle_.end());
      idle_bytes_ -= last->first;
      drop.push_back(last->second);
      idle_.erase(last);
    }
    return drop;
  }
  std::vector<void*> drain() {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<void*> all;
    for (auto& kv : idle_) all.push_back(kv.second);
    idle_.clear();
    idle_bytes_ = 0;
    return all;
  }
  size_t idle_bytes() {
    std::lock_guard<std::mutex> g(mu_);
    return idle_bytes_;
  }
  // capacity rs_host_alloc gives a fresh buffer of n bytes (2 MiB granules, so buffers
  // freed by one request fit the next request of similar size)
  static size_t granule(size_t n) { return (n + kGranule - 1) / kGranule * kGranule; }
  static constexpr size_t kGranule = 2u << 20;

 private:
  const size_t limit_;
  std::mutex mu_;
  std::multimap<size_t, void*> idle_;
  size_t idle_bytes_ = 0;
};

// How the host path cuts a call of `batch` stripes of n shards of S bytes into chunks of
// about `chunk_bytes` over all n shards, rotating through at most `slots` pipeline slots.
// A chunk is a block of spc whole stripes when a stripe is small (many stripes per H2D /
// launch / D2H), otherwise one column range of cw bytes of a single stripe: cw is a
// multiple of 4 KiB, at least 4 KiB, unless it is the whole shard; spc > 1 only when a
// whole stripe (shards pitched to 256 B) fits several times in a chunk.
struct ChunkGeometry {
  size_t cw = 0;      // columns (bytes per shard) per chunk
  int spc = 1;        // stripes per chunk
  size_t cpitch = 0;  // one shard in a slot's staging buffer
  size_t spitch = 0;  // one stripe there (n shards)
  size_t ncol = 0;    // column chunks per stripe
  size_t nblk = 0;    // stripe blocks per call
  int nslots = 0;     // slots in use: min(chunks, slots)
  // Small stripes move as one contiguous row range (rows that are not inputs ride
  // along). Larger chunks move one copy per run of consecutive shard indices: each copy
  // on a stream costs ~9 us of gap, so one copy per shard was much slower than one per
  // run.
  bool coalesce = false;
  size_t nchunks() const { return ncol * nblk; }
};

inline ChunkGeometry chunk_geometry(size_t S, int n, int batch, size_t chunk_bytes, int slots) {
  ChunkGeometry g;
  g.cw = S;
  const size_t nn = static_cast<size_t>(n);
  if (S * nn > chunk_bytes) {
    g.cw = std::max<size_t>(4096, chunk_bytes / nn / 4096 * 4096);
  } else {
    const size_t per = round_up(S, kPitchAlign) * nn;
    g.spc = static_cast<int>(
        std::min<size_t>(static_cast<size_t>(batch), std::max<size_t>(1, chunk_bytes / per)));
  }
  g.cpitch = round_up(g.cw, kPitchAlign);
  g.spitch = g.cpitch * nn;
  g.ncol = (S + g.cw - 1) / g.cw;
  g.nblk = (static_cast<size_t>(batch) + g.spc - 1) / g.spc;
  g.nslots = static_cast<int>(std::min<size_t>(g.nchunks(), static_cast<size_t>(slots)));
  g.coalesce = g.spitch <= (4u << 20);
  return g;
}

// Runs [first, last] of consecutive values in an index list (sorted here).
inline std::vector<std::pair<int, int>> index_runs(std::vector<int> v) {
  std::sort(v.begin(), v.end());
  std::vector<std::pair<int, int>> runs;
  for (int x : v) {
    if (!runs.empty() && runs.back().second + 1 == x) runs.back().second = x;
    else runs.push_back({x, x});
  }
  return runs;
}

// Decode's join/trim target (codec.go:67-77): data shard i's column c belongs at
// out[i*S + c] when that is below len (= min(originalSize, k*S)). The single-stripe
// host path writes it while the columns pass through the copy pool (a tee on the
// staging copies), instead of a separate k*S pass after the pipeline.
struct Join {
  uint8_t* out;
  size_t len;
  size_t S;  // full shard size (a column part's offset is added per part)
  int k;
};

// Tee target for shard i's columns [col, col+w) or {nullptr, 0}.
inline std::pair<uint8_t*, size_t> join_span(const Join* j, int i, size_t col, size_t w) {
  if (!j || i >= j->k) return {nullptr, 0};
  const size_t pos = static_cast<size_t>(i) * j->S + col;
  if (pos >= j->len) return {nullptr, 0};
  return {j->out + pos, std::min(w, j->len - pos)};
}

// Reconstruct's argument checks (upstream checkShards(shards, true)).
inline int check_lens(int n, const size_t* lens, bool nilok, size_t* S, int* npresent) {
  size_t size = 0;
  for (int i = 0; i < n; ++i)
    if (lens[i]) {
      size = lens[i];
      break;
    }
  if (size == 0) return RS_E_NO_DATA;
  int np = 0;
  for (int i = 0; i < n; ++i) {
    if (lens[i] != size && (lens[i] != 0 || !nilok)) return RS_E_SHARD_SIZE;
    np += lens[i] != 0;
  }
  *S = size;
  *npresent = np;
  return RS_OK;
}

// A stripe's shards as the batch calls group, class and build tables by them: the flags
// admission writes, and the only encoding of a wanted set (ReconstructSome) on the host path.
// A plain 0 / 1 presence mask (the encode batches') reads the same: every missing shard wanted.
constexpr uint8_t kShardWanted = 0;    // missing, to be rebuilt
constexpr uint8_t kShardPresent = 1;
constexpr uint8_t kShardUnwanted = 2;  // missing, neither written nor read

// A flag row as the table builders' arguments: present[i] and wanted[i], 0 / 1 each.
inline void shard_flags_split(const uint8_t* flags, size_t count, uint8_t* present, uint8_t* wanted) {
  for (size_t i = 0; i < count; ++i) {
    present[i] = flags[i] == kShardPresent;
    wanted[i] = flags[i] == kShardWanted;
  }
}

// Whether one stripe of a reconstruct (n shards, k of them data) is to run. wanted: n flags
// (nonzero = wanted; flags on present shards count for nothing), or null: every missing shard.
// In upstream's order: check_lens' status, RS_E_TOO_FEW_SHARDS below k present shards, nothing
// to do (run false, status RS_OK) when no missing shard is wanted and nothing is compared
// (!verify), RS_E_ARG for a NULL shard among those the call touches -- the present ones and the
// wanted missing ones; an unwanted missing shard may be NULL. With verify, a stripe of exactly k
// present shards that wants nothing has no row either: run false, status RS_OK, and `flags`
// and S are still written (decode's join copies its data shards). flags: n of kShard*.
struct StripeAdmission {
  int status = RS_OK;  // the stripe's own when it does not run
  bool run = false;
  size_t S = 0;
};
inline StripeAdmission admit_stripe(int n, int k, const uint8_t* const* shards, const size_t* lens,
                                    const uint8_t* wanted, bool verify, uint8_t* flags) {
  StripeAdmission a;
  int np = 0;
  if ((a.status = check_lens(n, lens, true, &a.S, &np))) return a;
  if (np < k) {
    a.status = RS_E_TOO_FEW_SHARDS;
    return a;
  }
  auto want = [&](int i) { return !wanted || wanted[i]; };
  int w = 0;
  for (int i = 0; i < n; ++i) w += !lens[i] && want(i);
  if (w == 0 && !verify) return a;
  for (int i = 0; i < n; ++i)
    if (!shards[i] && (lens[i] || want(i))) {
      a.status = RS_E_ARG;
      return a;
    }
  for (int i = 0; i < n; ++i) flags[i] = lens[i] ? kShardPresent : want(i) ? kShardWanted : kShardUnwanted;
  a.run = w + (np - k) > 0;
  return a;
}

// Stripes grouped by (S, flag row): each group shares one table set and one pipeline.
struct BatchGroups {
  std::map<std::string, std::vector<int>> by_key;
  std::vector<int> stripes;  // every stripe added, in the order of the calls
  void add(size_t S, const uint8_t* present, int n, int b) {
    std::string key(reinterpret_cast<const char*>(&S), sizeof S);
    key.append(reinterpret_cast<const char*>(present), n);
    by_key[key].push_back(b);
    stripes.push_back(b);
  }
  static size_t shard_size(const std::string& key) {
    size_t S;
    std::memcpy(&S, key.data(), sizeof S);
    return S;
  }
  static const uint8_t* present(const std::string& key) {
    return reinterpret_cast<const uint8_t*>(key.data() + sizeof(size_t));
  }
};

// How a batch call's runnable stripes reach the GPU. Two or more groups, with the ragged
// pipeline allowed: one ragged run over `ids`, every runnable stripe in ascending call order.
// Otherwise one uniform pipeline per entry of `groups`, in by_key's order (none when the call
// has nothing to run).
struct BatchRoute {
  bool ragged = false;
  std::vector<int> ids;
  std::vector<const std::pair<const std::string, std::vector<int>>*> groups;
};
inline BatchRoute batch_route(const BatchGroups& g, bool ragged_allowed) {
  BatchRoute r;
  r.ragged = g.by_key.size() >= 2 && ragged_allowed;
  if (r.ragged) {
    // the callers add their stripes in ascending order: then this is a copy, not a sort
    r.ids = g.stripes;
    if (!std::is_sorted(r.ids.begin(), r.ids.end())) std::sort(r.ids.begin(), r.ids.end());
  } else {
    for (const auto& kv : g.by_key) r.groups.push_back(&kv);
  }
  return r;
}

}  // namespace callfs
