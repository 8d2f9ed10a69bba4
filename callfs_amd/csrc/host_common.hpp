// What both pipelines of the host-memory path (host_uniform.hpp, host_ragged.hpp) stand on:
// the environment knobs, the lane scope of a call, the completion flag of the in-place
// kernels and the join step of the zero-copy paths. Included by rs_host.cpp only.
#pragma once

#include <chrono>
#include <thread>

#include "rs_internal.hpp"
#include "sums_host.hpp"

namespace callfs {
namespace {

// Pipeline depth (slots per lane): CALLFS_RS_SLOTS overrides, 2..kMaxSlots.
int pipeline_slots() {
  static const int v = [] {
    const char* e = std::getenv("CALLFS_RS_SLOTS");
    const int x = e ? std::atoi(e) : 3;
    return std::max(2, std::min(kMaxSlots, x));
  }();
  return v;
}
// Column chunk: about this many bytes over all n shards per pipeline step
// (CALLFS_RS_CHUNK_BYTES overrides; DESIGN.md §7.4 has the sweep).
size_t chunk_bytes() {
  static const size_t v = [] {
    const char* e = std::getenv("CALLFS_RS_CHUNK_BYTES");
    const long long x = e ? std::atoll(e) : 0;
    return x >= (64 << 10) ? static_cast<size_t>(x) : (16u << 20);
  }();
  return v;
}

// Calls moving at most this many staging bytes (n shards rounded to 16 B, all stripes)
// take the one-dispatch small path (CALLFS_RS_SMALL_MAX_BYTES overrides; 0 turns it off).
size_t small_max_bytes() {
  static const size_t v = [] {
    const char* e = std::getenv("CALLFS_RS_SMALL_MAX_BYTES");
    return e ? static_cast<size_t>(std::strtoull(e, nullptr, 0)) : (2u << 20);
  }();
  return v;
}

// CALLFS_RS_INPLACE_PIPELINE=1: calls above the small limit run the chunk pipeline with
// in-place kernels on host-coherent staging instead of H2D / kernel / D2H (A/B)
bool inplace_pipeline() {
  static const bool on = [] {
    const char* e = std::getenv("CALLFS_RS_INPLACE_PIPELINE");
    return e && *e == '1';
  }();
  return on;
}

// A batch call whose runnable stripes differ in shard size or erasure pattern runs as one
// ragged pipeline (host_ragged.hpp) instead of one uniform pipeline per (S, mask) group.
// CALLFS_RS_RAGGED_BATCH=0 keeps every call on the per-group route (A/B and fallback).
bool ragged_batch() {
  static const bool on = [] {
    const char* e = std::getenv("CALLFS_RS_RAGGED_BATCH");
    return !(e && *e == '0');
  }();
  return on;
}

// Where a checksummed codec batch hashes its whole-stripe items (sums_table.hpp has the rule):
// CALLFS_RS_SUMS_DEVICE=0 the copy pool's threads always, =1 the device always, else `auto`.
SumsKnob sums_device_knob() {
  static const SumsKnob v = [] {
    const char* e = std::getenv("CALLFS_RS_SUMS_DEVICE");
    if (e && e[0] == '0' && !e[1]) return SumsKnob::kHost;
    if (e && e[0] == '1' && !e[1]) return SumsKnob::kDevice;
    return SumsKnob::kAuto;
  }();
  return v;
}

// Zero-copy: when every caller buffer lies in rs_host_alloc memory (page-locked and
// mapped into the device's address space at the same address), the kernels read and
// write the caller's bytes over PCIe in one launch set over the whole call -- no
// staging copies, no chunk pipeline, nothing for the CPU but the join of present
// data shards. RS(10,4) 64 MiB: 43.7 GiB/s vs 36.7 for H2D + launch + D2H
// (tests/perf/zerocopy_probe.py).
// Threshold: 48 KiB per shard over the call (S x batch), i.e. 48 KiB x n over all n
// shards. Below it the one-dispatch path on the library's coherent staging is faster;
// tools/jobs.sh zc_threshold (profiles/r04/zc_threshold/zc.jsonl, GiB/s enc / dec, 1 thread,
// zero-copy vs one-dispatch): RS(4,2) 128 KiB objects 4.6 / 4.2 vs 6.2 / 5.9, 256 KiB
// 8.7 / 7.7 vs 5.3 / 5.3; RS(10,4) 384 KiB 9.6 / 8.9 vs 9.0 / 9.1, 512 KiB 11.7 / 11.4 vs
// 8.0 / 10.0; RS(16,4) 512 KiB 11.2 / 9.1 vs 10.9 / 9.2, 1 MiB 20.9 / 17.1 vs 10.8 / 14.6.
// CALLFS_RS_ZERO_COPY_MIN_BYTES sets it in bytes over all n shards instead.
unsigned long long zero_copy_min(unsigned long long n) {
  static const long long zc_env = [] {
    const char* e = std::getenv("CALLFS_RS_ZERO_COPY_MIN_BYTES");
    return e ? static_cast<long long>(std::strtoull(e, nullptr, 0)) : -1LL;
  }();
  return zc_env >= 0 ? static_cast<unsigned long long>(zc_env) : (48ull << 10) * n;
}

struct LaneGuard {
  rs_ctx* ctx;
  Device* dev;
  Lane* lane;
  ~LaneGuard() {
    if (lane) ctx->release(dev, lane);
  }
};

// Runs fn(lane) on a lane of `dev` held for the call. Any return but RS_OK / RS_E_CORRUPT may
// have left work in flight: the slots' streams are drained before the next caller gets the lane.
template <class F>
int with_lane(rs_ctx* ctx, Device* dev, F fn) {
  LaneGuard lg{ctx, dev, ctx->acquire(dev)};
  if (!lg.lane) return RS_E_HIP;
  const int rc = fn(*lg.lane);
  if (rc != RS_OK && rc != RS_E_CORRUPT)
    for (Slot& sl : lg.lane->slot) {
      if (sl.stream) (void)hipStreamSynchronize(sl.stream);
      sl.pending = false;
    }
  return rc;
}

// The completion flag of the in-place kernels (rs_apply_small, rs_apply_small_ragged): the
// last launch group of a chunk releases the slot's sequence number into an int at done_off
// of the slot's coherent staging once all its blocks have ended. A mistake here hangs a
// caller, so both in-place transports go through ensure / arm / wait below.
// Host spin on the flag: true once *flag == want, false after `us` microseconds.
constexpr int kSmallSpinUs = 2000;
bool spin_until(const int* flag, int want, int us) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned i = 0;; ++i) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == want) return true;
    if ((i & 63u) == 63u &&
        std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(us))
      return false;
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
  }
}

// The slot's staging up to the flag's 256 bytes at done_off, and its zeroed counter.
int done_flag_ensure(Slot& sl, size_t done_off) {
  int rc;
  if ((rc = sl.small.ensure(done_off + 256))) return rc;
  if (!sl.small_counter.p) {
    if ((rc = sl.small_counter.ensure(256))) return rc;
    HIPCHK(hipMemset(sl.small_counter.p, 0, 256));
  }
  return RS_OK;
}

// Before a chunk's launches: the next sequence number in sl.small_seq and the flag cleared (a
// fresh or moved buffer holds whatever it held). Returns the flag, for the last group's launch.
int* done_flag_arm(Slot& sl, size_t done_off) {
  int* done = reinterpret_cast<int*>(static_cast<uint8_t*>(sl.small.p) + done_off);
  sl.small_seq = sl.small_seq >= 0x3fffffff ? 1 : sl.small_seq + 1;  // never 0
  __atomic_store_n(done, 0, __ATOMIC_RELEASE);
  return done;
}

// Until the chunk armed last has landed: ~5 us sooner than the runtime's completion signal;
// past kSmallSpinUs the stream wait, which also reports a faulted kernel.
int done_flag_wait(Slot& sl, size_t done_off) {
  const int* done = reinterpret_cast<const int*>(static_cast<const uint8_t*>(sl.small.p) + done_off);
  if (!spin_until(done, sl.small_seq, kSmallSpinUs)) HIPCHK(hipStreamSynchronize(sl.stream));
  return RS_OK;
}

// A direct call's joins around its launches (recorded in sl.done): the present shards' segments
// run while the kernels do, the rebuilt shards' once they have landed.
int join_around_launch(rs_ctx* ctx, Slot& sl, const std::vector<CopyPool::Seg>& present,
                       const std::vector<CopyPool::Seg>& rebuilt) {
  ctx->pool.run(present);
  HIPCHK(hipEventSynchronize(sl.done));
  ctx->pool.run(rebuilt);
  return RS_OK;
}

}  // namespace
}  // namespace callfs
