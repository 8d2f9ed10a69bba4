// What the C ABI's translation units share (include/callfs_rs.h; rs_context.cpp,
// rs_host.cpp, rs_plan.cpp). Internal to the library.
//
//  * rs_ctx     — selected devices, each with a pool of Lanes and a cache of decode
//                 tables keyed by (k, m, presence mask); the rs_host_alloc registry and pool.
//  * Lane       — kMaxSlots Slots: one HIP stream each plus grow-only device/pinned
//                 buffers: the pitched shard workspace used by the host-memory entry
//                 points, pointer tables and coefficient tables for one-shot launches.
//  * Tables     — the launch groups of one (k, m, presence mask): coefficient tables per
//                 group of up to kMaxRowsPerLaunch output rows.
//  * MetaLayout — where one set of launches' pointer tables, coefficient tables and status
//                 words sit in one device buffer; fill_meta / group_args / launch_groups.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/callfs_rs.h"
#include "bitslice.hpp"
#include "copy_pool.hpp"
#include "dispatch.hpp"
#include "gf256.hpp"
#include "host_path.hpp"
#include "rs_kernels.hpp"

#define HIPCHK(x)                           \
  do {                                      \
    if ((x) != hipSuccess) return RS_E_HIP; \
  } while (0)

namespace callfs {

// Restores the calling thread's current HIP device on scope exit: entry points select
// the device they work on, and a caller's later default-device work (torch, HIP) must
// not land on another GPU because of a codec call.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

constexpr int kMaxLanesPerDevice = 8;

inline int check_profile(int k, int m) {
  if (k < 1 || m < 1) return RS_E_INVALID_PROFILE;
  if (k + m > 256) return RS_E_UNSUPPORTED;
  return RS_OK;
}

// ---- coefficient tables -----------------------------------------------------------

// One launch group: up to kMaxRowsPerLaunch output rows over the same k inputs.
struct Group {
  std::vector<int> shard;     // shard index per row
  uint32_t verify_mask = 0;   // bit r: compare row r (Verify) instead of storing it
  std::vector<uint32_t> tabs; // [k][R][5] v_perm tables
  std::vector<uint8_t> ltabs;  // [k][32][W] LDS nibble tables (used for R >= 5)
  // the group's bit-sliced kernel (bitslice.hpp; compiled on demand), R >= kBitsliceMinRows
  std::shared_ptr<bs::Kernel> bsk;
};

struct Tables {
  int k = 0, m = 0;
  std::vector<int> valid;
  std::vector<int> missing;
  std::vector<int> check;
  std::vector<Group> groups;
};

class TableCache {
 public:
  // verify=false drops the check rows (plain Reconstruct). wanted (k+m flags, or null: every
  // missing shard): a missing shard whose flag is clear gets no row (ReconstructSome); a
  // wanted set that names every missing shard shares the null entry. Null: a singular matrix.
  std::shared_ptr<const Tables> get(int k, int m, const uint8_t* present, bool verify,
                                    const uint8_t* wanted = nullptr);

 private:
  static constexpr size_t kCap = 4096;
  std::mutex mu_;
  std::unordered_map<std::string, std::shared_ptr<const Tables>> map_;
};

// ---- buffers ---------------------------------------------------------------------------

// A grow-only buffer: ensure(n) keeps it when it is large enough, else frees and
// reallocates (contents are not kept). Mem says where the bytes live.
template <class Mem>
struct Buffer {
  void* p = nullptr;
  size_t cap = 0;
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { release(); }
  int ensure(size_t n) {
    if (n <= cap) return RS_OK;
    release();
    n = std::max(n, Mem::kFloor);
    if (Mem::alloc(&p, n) != hipSuccess) {
      p = nullptr;
      return RS_E_NOMEM;
    }
    cap = n;
    return RS_OK;
  }
  void release() {
    if (p) Mem::free(p);
    p = nullptr;
    cap = 0;
  }
};

struct DeviceMem {
  static constexpr size_t kFloor = 0;
  static hipError_t alloc(void** p, size_t n) { return hipMalloc(p, n); }
  static void free(void* p) { (void)hipFree(p); }
};

// Pinned staging the copy engines move. Non-coherent: DMA into the default (coherent,
// fine-grained) pinned memory ran at 9 GB/s for 4 MiB D2H copies and 34-41 GB/s at 64 MiB,
// against 50 / 57 GB/s here (tools/host_ceilings.cpp). The host reads
// staging only after the slot's event has completed, so coherence during the copy is
// never needed. CALLFS_RS_PINNED_COHERENT switches back (A/B).
struct StagingMem {
  static constexpr size_t kFloor = 0;
  static hipError_t alloc(void** p, size_t n) {
    static const unsigned flags =
        std::getenv("CALLFS_RS_PINNED_COHERENT") ? hipHostMallocDefault : hipHostMallocNonCoherent;
    return hipHostMalloc(p, n, flags);
  }
  static void free(void* p) { (void)hipHostFree(p); }
};

// Host-coherent pinned memory that kernels read and write in place (the one-dispatch
// small-call path): the CPU fills it between calls, so device caches must not keep its
// lines across launches (as for rs_host_alloc buffers).
struct CoherentMem {
  static constexpr size_t kFloor = 64u << 10;
  static hipError_t alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocCoherent); }
  static void free(void* p) { (void)hipHostFree(p); }
};

using DevBuf = Buffer<DeviceMem>;
using HostBuf = Buffer<StagingMem>;
using CoherentBuf = Buffer<CoherentMem>;

// `bytes` of `h` into `d` on `device` (made current): what a plan's device buffer holds.
inline int upload(DevBuf& d, int device, const void* h, size_t bytes) {
  HIPCHK(hipSetDevice(device));
  if (const int rc = d.ensure(bytes)) return rc;
  HIPCHK(hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice));
  return RS_OK;
}

// Layout facts the kernel dispatch keys its tile order on (ApplyArgs addr_tz,
// stripe_stride).
struct LayoutHint {
  int addr_tz = 0;
  uint64_t stripe_stride = 0;
  uint32_t in_misalign = 0;
  uint32_t out_misalign = 0;  // over every launch group's output pointers
};

// One pipeline stage of the host-memory path: a stream, a pinned chunk buffer and its
// device mirror ([n][cpitch]), and the pointer/coefficient tables for launches on it.
struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  DevBuf dev;
  HostBuf host;
  DevBuf meta;
  HostBuf hmeta;
  std::shared_ptr<const Tables> meta_tables;  // what `meta` currently holds
  size_t meta_pitch = 0;
  int meta_spc = 0;
  LayoutHint meta_hint;  // of the pointers in `meta`
  void* meta_base = nullptr;
  HostBuf hstat;         // per-stripe verify flags of the chunk in flight
  // one-dispatch small calls: staging the kernel works on in place (+ status words),
  // and the v_perm tables of the tables set it was last used with, per launch group
  CoherentBuf small;
  DevBuf small_counter;  // finished-block counter of the completion flag
  int small_seq = 0;     // sequence number of the last small call on this slot
  DevBuf small_tabs;
  std::shared_ptr<const Tables> small_tables;
  std::vector<size_t> small_tab_off;
  bool pending = false;  // a chunk's outputs wait in staging
  int b0 = 0, count = 0;  // its stripes
  size_t off = 0, width = 0;  // and columns
  size_t rag_chunk = 0;       // the chunk in flight (host_chunks.hpp run_chunk_pipeline)
};

constexpr int kMaxSlots = 6;

struct Lane {
  Slot slot[kMaxSlots];
  // Pattern tables of the last ragged run on this lane, keyed by the run's
  // profile and pattern list: the launch groups' arenas and compare masks for the staged and
  // direct transports, the v_perm blocks for the in-place one. A stream of batches of one
  // profile and pattern list (every encode batch) uploads nothing after the first.
  DevBuf rag_tabs, rag_small_tabs;
  std::string rag_key, rag_small_key;
};

struct Device {
  int id = 0;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::unique_ptr<Lane>> lanes;
  std::vector<Lane*> free_lanes;
};

// Device-side layout of everything one set of launches needs, packed into one buffer.
struct MetaLayout {
  size_t in_off = 0, status_off = 0, total = 0;
  std::vector<size_t> out_off, tab_off, ltab_off;
};

MetaLayout meta_layout(const Tables& t, int batch);

// Fill host staging for the meta buffer. shard_ptr(b, i) gives stripe b's shard i.
// Returns the layout hint: shard_addr_tz over the shards stripe 0's launches touch, and
// the stripe stride when every stripe sits at the same distance from the previous one.
template <class F>
LayoutHint fill_meta(const Tables& t, const MetaLayout& L, int batch, uint8_t* h, F shard_ptr) {
  std::memset(h + L.status_off, 0, sizeof(int) * static_cast<size_t>(batch));
  auto* in = reinterpret_cast<const uint8_t**>(h + L.in_off);
  uint32_t misalign = 0, out_misalign = 0;
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < t.k; ++i) {
      const uint8_t* p = shard_ptr(b, t.valid[i]);
      in[static_cast<size_t>(b) * t.k + i] = p;
      misalign |= static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u;
    }
  for (size_t gi = 0; gi < t.groups.size(); ++gi) {
    const Group& g = t.groups[gi];
    auto* out = reinterpret_cast<uint8_t**>(h + L.out_off[gi]);
    const size_t R = g.shard.size();
    for (int b = 0; b < batch; ++b)
      for (size_t r = 0; r < R; ++r) {
        out[b * R + r] = const_cast<uint8_t*>(shard_ptr(b, g.shard[r]));
        out_misalign |= static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out[b * R + r])) & 15u;
      }
    std::memcpy(h + L.tab_off[gi], g.tabs.data(), g.tabs.size() * sizeof(uint32_t));
    std::memcpy(h + L.ltab_off[gi], g.ltabs.data(), g.ltabs.size());
  }
  std::vector<const void*> s0;
  for (int i : t.valid) s0.push_back(shard_ptr(0, i));
  for (const Group& g : t.groups)
    for (int i : g.shard) s0.push_back(shard_ptr(0, i));
  LayoutHint hint;
  hint.in_misalign = misalign;
  hint.out_misalign = out_misalign;
  hint.addr_tz = shard_addr_tz(s0.data(), static_cast<int>(s0.size()));
  if (batch > 1) {
    const int v = t.valid[0];
    auto addr = [&](int b) { return reinterpret_cast<uintptr_t>(shard_ptr(b, v)); };
    const uint64_t stride = addr(1) - addr(0);
    bool regular = true;
    for (int b = 2; b < batch && regular; ++b) regular = addr(b) - addr(b - 1) == stride;
    if (regular) hint.stripe_stride = stride;
  }
  return hint;
}

// The launch arguments of group gi of tables `t` laid out by `L` in device buffer `d`.
ApplyArgs group_args(const Tables& t, const MetaLayout& L, size_t gi, int batch, uint8_t* d,
                     size_t S, int status_stride, const LayoutHint& hint);

// Group gi of ng's share of a launch's events: the first group's first dispatch records
// ev.start, the last group's last ev.stop.
inline LaunchEvents group_events(const LaunchEvents& ev, size_t gi, size_t ng) {
  LaunchEvents g;
  g.start = gi == 0 ? ev.start : nullptr;
  g.stop = gi + 1 == ng ? ev.stop : nullptr;
  return g;
}

// orders: per launch group, a TileOrder from rs_plan_tune or -1 (the rule); null = rule.
hipError_t launch_groups(const Tables& t, const MetaLayout& L, int batch, uint8_t* d, size_t S,
                         hipStream_t s, int status_stride, const LayoutHint& hint,
                         const std::vector<int>* orders = nullptr, LaunchEvents ev = {});

}  // namespace callfs

// ---- context ------------------------------------------------------------------------

struct rs_ctx {
  std::vector<std::unique_ptr<callfs::Device>> devs;
  std::atomic<unsigned> rr{0};
  callfs::TableCache cache;
  callfs::CopyPool pool;
  callfs::PinnedRegistry pinned;
  callfs::HostPool host_pool;
  // rs_host_counters_read: monotonic, relaxed
  std::atomic<uint64_t> n_calls{0}, n_chunks{0}, n_launches{0}, n_copies{0}, n_ragged_calls{0};

  rs_ctx();
  ~rs_ctx();
  callfs::Device* device(int id);
  // a free lane of the device (waits for one when all kMaxLanesPerDevice are busy); null
  // on a HIP error
  callfs::Lane* acquire(callfs::Device* d);
  void release(callfs::Device* d, callfs::Lane* l);
};
