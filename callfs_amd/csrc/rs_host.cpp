// The host-memory path of the C ABI (include/callfs_rs.h): the per-object calls
// (Codec.Encode / Decode ends, Encode, Reconstruct, Verify) and the batch calls.
//
// The control flow and error precedence follow codec.go:21-78 and the upstream
// reedsolomon methods it calls (Split/Encode at :31/:36, Reconstruct at :55, Verify at
// :59). A call's stripes go through one of two ways: zero-copy launches on the caller's
// rs_host_alloc buffers (run_direct), or the chunk pipeline (run_chunks) over a lane's
// slots, whose chunks a transport sends to the GPU and awaits -- staged (H2D / kernels /
// D2H) or in place on host-coherent staging (one dispatch per launch group).
#include <chrono>
#include <thread>

#include "codec_batch.hpp"
#include "ragged_chunks.hpp"
#include "rs_internal.hpp"

using namespace callfs;

namespace {

struct LaneGuard {
  rs_ctx* ctx;
  Device* dev;
  Lane* lane;
  ~LaneGuard() {
    if (lane) ctx->release(dev, lane);
  }
};

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

// Host spin on a flag a kernel releases with a system-scope store (rs_apply_small):
// true once *flag == want, false after `us` microseconds.
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

// One host-memory call over `batch` stripes that share one table set and one shard size
// S. in(b, i) / out(b, i) give host buffers by stripe and shard index. stripe_status
// (nullable, `batch` ints) receives 1 for stripes whose verify rows mismatched. `join`
// (nullable, one Join per stripe; host_path.hpp) is written while the columns pass through
// the copy pool; col0 is this call's first column in the whole object (a column part of a
// split object).
template <class InF, class OutF>
struct HostCall {
  rs_ctx* ctx;
  const std::shared_ptr<const Tables>& tp;
  size_t S;
  int batch;
  InF& in;
  OutF& out;
  int* stripe_status;
  const Join* join;
  size_t col0;
  std::vector<int> ins;  // the shards read: valid, then the compared ones

  const Tables& t() const { return *tp; }
  const std::vector<int>& outs() const { return tp->missing; }  // the shards written
  int n() const { return tp->k + tp->m; }
  bool verify() const { return !tp->check.empty(); }
  const Join* join_of(int b) const { return join ? join + b : nullptr; }
  // marks the stripes from b0 whose status word is set; true when any is
  bool scan_status(const int* st, int b0, int count) const {
    bool corrupt = false;
    for (int b = 0; b < count; ++b)
      if (st[b]) {
        corrupt = true;
        if (stripe_status) stripe_status[b0 + b] = 1;
      }
    return corrupt;
  }
};

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
// (Round 2's 128 KiB over all shards predates the one-dispatch path.)
// CALLFS_RS_ZERO_COPY_MIN_BYTES sets it in bytes over all n shards instead.
unsigned long long zero_copy_min(unsigned long long n) {
  static const long long zc_env = [] {
    const char* e = std::getenv("CALLFS_RS_ZERO_COPY_MIN_BYTES");
    return e ? static_cast<long long>(std::strtoull(e, nullptr, 0)) : -1LL;
  }();
  return zc_env >= 0 ? static_cast<unsigned long long>(zc_env) : (48ull << 10) * n;
}

template <class InF, class OutF>
bool direct_ok(const HostCall<InF, OutF>& c) {
  const unsigned long long n = static_cast<unsigned long long>(c.n());
  const unsigned long long zc_min = zero_copy_min(n);
  const PinnedRegistry& pinned = c.ctx->pinned;
  bool direct = !pinned.empty() && static_cast<unsigned long long>(c.S) * n * c.batch >= zc_min;
  for (int b = 0; direct && b < c.batch; ++b) {
    for (int i : c.ins) direct = direct && pinned.contains(c.in(b, i), c.S);
    for (int i : c.outs()) direct = direct && pinned.contains(c.out(b, i), c.S);
  }
  for (int b = 0; direct && c.join && b < c.batch; ++b)
    direct = c.join[b].len == 0 || pinned.contains(c.join[b].out, c.join[b].len);
  return direct;
}

template <class InF, class OutF>
int run_direct(const HostCall<InF, OutF>& c, Slot& sl) {
  const Tables& t = c.t();
  const int batch = c.batch;
  const MetaLayout DL = meta_layout(t, batch);
  int rc;
  if ((rc = sl.meta.ensure(DL.total)) || (rc = sl.hmeta.ensure(DL.total)) ||
      (rc = sl.hstat.ensure(sizeof(int) * batch)))
    return rc;
  sl.meta_tables = nullptr;  // the staged path refills its tables next time
  std::vector<char> is_out(c.n(), 0);
  for (int i : c.outs()) is_out[i] = 1;
  const LayoutHint hint = fill_meta(t, DL, batch, static_cast<uint8_t*>(sl.hmeta.p), [&](int b, int i) {
    return is_out[i] ? static_cast<const uint8_t*>(c.out(b, i)) : c.in(b, i);
  });
  auto* meta = static_cast<uint8_t*>(sl.meta.p);
  HIPCHK(hipMemcpyAsync(meta, sl.hmeta.p, DL.total, hipMemcpyHostToDevice, sl.stream));
  HIPCHK(launch_groups(t, DL, batch, meta, c.S, sl.stream, 1, hint));
  if (c.verify())
    HIPCHK(hipMemcpyAsync(sl.hstat.p, meta + DL.status_off, sizeof(int) * batch,
                          hipMemcpyDeviceToHost, sl.stream));
  HIPCHK(hipEventRecord(sl.done, sl.stream));
  c.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
  c.ctx->n_launches.fetch_add(t.groups.size(), std::memory_order_relaxed);
  c.ctx->n_copies.fetch_add(c.verify() ? 2 : 1, std::memory_order_relaxed);
  // decode's join: present data shards go to `out` while the kernels run,
  // reconstructed ones once they have landed
  auto join_segs = [&](bool present) {
    std::vector<CopyPool::Seg> js_segs;
    for (int b = 0; c.join && b < batch; ++b)
      for (int i = 0; i < t.k; ++i) {
        if (static_cast<bool>(is_out[i]) == present) continue;
        const auto js = join_span(c.join_of(b), i, c.col0, c.S);
        if (js.first)
          js_segs.push_back({js.first, present ? c.in(b, i) : c.out(b, i), js.second});
      }
    c.ctx->pool.run(js_segs);
  };
  join_segs(true);
  HIPCHK(hipEventSynchronize(sl.done));
  join_segs(false);
  const bool corrupt = c.verify() && c.scan_status(static_cast<const int*>(sl.hstat.p), 0, batch);
  return corrupt ? RS_E_CORRUPT : RS_OK;
}

// ---- the chunk pipeline -----------------------------------------------------------------

// Work is cut into chunks (host_path.hpp ChunkGeometry) that rotate through the lane's
// slots. Per chunk: copy-pool copies of the input shards into the slot's staging
// ([stripe][n][cpitch]), then the transport sends the chunk to the GPU on the slot's
// stream; the CPU copies chunk j in while the GPU works on chunks j-1 and j-2, and copies
// chunk j-nslots out. A transport gives:
//   prepare(slot)         buffers and tables of one slot, once per call
//   staging(slot)         the slot's staging buffer, pitched as g.cpitch / g.spitch
//   send(slot, cnt, w)    enqueue the chunk in staging: cnt stripes, w bytes per shard
//   wait(slot)            until the chunk sent last has landed back in staging
//   status(slot)          its cnt per-stripe verify words
// Returns RS_OK, RS_E_CORRUPT (some stripe mismatched) or an error.
template <class Transport, class InF, class OutF>
int run_chunks(const HostCall<InF, OutF>& c, Lane& L, const ChunkGeometry& g, Transport& tr) {
  for (int si = 0; si < g.nslots; ++si) {
    const int rc = tr.prepare(L.slot[si]);
    if (rc) return rc;
    L.slot[si].pending = false;
  }
  bool corrupt = false;
  std::vector<CopyPool::Seg> segs;
  // Waits for the slot's chunk and appends its output copies to `segs` (run by the
  // caller together with the next chunk's input copies: one pool job per step; the
  // slot's input and output rows are disjoint).
  auto drain = [&](Slot& sl) -> int {
    if (!sl.pending) return RS_OK;
    const int rc = tr.wait(sl);
    if (rc) return rc;
    if (c.verify() && c.scan_status(tr.status(sl), sl.b0, sl.count)) corrupt = true;
    uint8_t* h = tr.staging(sl);
    for (int b = 0; b < sl.count; ++b)
      for (int i : c.outs()) {
        const auto tee = join_span(c.join_of(sl.b0 + b), i, c.col0 + sl.off, sl.width);
        segs.push_back({c.out(sl.b0 + b, i) + sl.off, h + g.spitch * b + g.cpitch * i, sl.width,
                        tee.first, tee.second});
      }
    sl.pending = false;
    return RS_OK;
  };
  const size_t nchunks = g.nchunks(), nslots = static_cast<size_t>(g.nslots);
  for (size_t j = 0; j < nchunks; ++j) {
    Slot& sl = L.slot[j % nslots];
    segs.clear();
    int rc = drain(sl);
    if (rc) return rc;
    const int b0 = static_cast<int>(j / g.ncol) * g.spc;
    const int cnt = std::min(g.spc, c.batch - b0);
    const size_t off = (j % g.ncol) * g.cw, w = std::min(g.cw, c.S - off);
    uint8_t* h = tr.staging(sl);
    for (int b = 0; b < cnt; ++b)
      for (int i : c.ins) {
        const auto tee = join_span(c.join_of(b0 + b), i, c.col0 + off, w);
        segs.push_back({h + g.spitch * b + g.cpitch * i, c.in(b0 + b, i) + off, w, tee.first,
                        tee.second});
      }
    c.ctx->pool.run(segs);
    if ((rc = tr.send(sl, cnt, w))) return rc;
    c.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
    c.ctx->n_launches.fetch_add(c.t().groups.size(), std::memory_order_relaxed);
    sl.pending = true;
    sl.b0 = b0;
    sl.count = cnt;
    sl.off = off;
    sl.width = w;
  }
  for (size_t j = nchunks - nslots; j < nchunks; ++j) {
    segs.clear();
    const int rc = drain(L.slot[j % nslots]);
    if (rc) return rc;
    c.ctx->pool.run(segs);
  }
  return corrupt ? RS_E_CORRUPT : RS_OK;
}

// Staged: H2D of the input shards, the kernel groups on the slot's device mirror, D2H of
// the written shards (and of the per-stripe status words when there are verify rows),
// then the slot's event.
struct StagedTransport {
  const std::shared_ptr<const Tables>& tp;
  const ChunkGeometry& g;
  const MetaLayout ML;
  // one copy per run of consecutive shard indices (or one over [lo, hi] when g.coalesce)
  const std::vector<std::pair<int, int>> in_runs, out_runs;
  const bool verify;
  rs_ctx* const ctx;  // its copies counter

  StagedTransport(rs_ctx* context, const std::shared_ptr<const Tables>& tables,
                  const ChunkGeometry& geo, const std::vector<int>& ins)
      : tp(tables), g(geo), ML(meta_layout(*tables, geo.spc)), in_runs(index_runs(ins)),
        out_runs(index_runs(tables->missing)), verify(!tables->check.empty()), ctx(context) {}

  int prepare(Slot& sl) {
    const size_t spitch = g.spitch, cpitch = g.cpitch;
    int rc;
    if ((rc = sl.dev.ensure(spitch * g.spc)) || (rc = sl.host.ensure(spitch * g.spc)) ||
        (rc = sl.meta.ensure(ML.total)) || (rc = sl.hmeta.ensure(ML.total)) ||
        (rc = sl.hstat.ensure(sizeof(int) * g.spc)))
      return rc;
    if (sl.meta_tables != tp || sl.meta_pitch != cpitch || sl.meta_spc != g.spc ||
        sl.meta_base != sl.dev.p) {
      auto* base = static_cast<uint8_t*>(sl.dev.p);
      sl.meta_hint = fill_meta(*tp, ML, g.spc, static_cast<uint8_t*>(sl.hmeta.p),
                               [&](int b, int i) { return base + spitch * b + cpitch * i; });
      HIPCHK(hipMemcpyAsync(sl.meta.p, sl.hmeta.p, ML.total, hipMemcpyHostToDevice, sl.stream));
      count_copies(1);
      sl.meta_tables = tp;
      sl.meta_pitch = cpitch;
      sl.meta_spc = g.spc;
      sl.meta_base = sl.dev.p;
    }
    return RS_OK;
  }
  uint8_t* staging(Slot& sl) const { return static_cast<uint8_t*>(sl.host.p); }
  const int* status(Slot& sl) const { return static_cast<const int*>(sl.hstat.p); }
  int wait(Slot& sl) const {
    HIPCHK(hipEventSynchronize(sl.done));
    return RS_OK;
  }
  void count_copies(size_t n) const { ctx->n_copies.fetch_add(n, std::memory_order_relaxed); }

  // the chunk's rows in `runs` from `src` to `dst` (both pitched like staging)
  int copy_rows(Slot& sl, const std::vector<std::pair<int, int>>& runs, uint8_t* dst,
                const uint8_t* src, int cnt, size_t w, hipMemcpyKind kind) const {
    const size_t spitch = g.spitch, cpitch = g.cpitch;
    if (g.coalesce) {
      const int lo = runs.front().first, hi = runs.back().second;
      const size_t bytes = spitch * (cnt - 1) + cpitch * (hi - lo) + w;
      HIPCHK(hipMemcpyAsync(dst + cpitch * lo, src + cpitch * lo, bytes, kind, sl.stream));
      count_copies(1);
      return RS_OK;
    }
    for (int b = 0; b < cnt; ++b)
      for (const auto& r : runs) {
        const size_t o = spitch * b + cpitch * r.first;
        HIPCHK(hipMemcpyAsync(dst + o, src + o, cpitch * (r.second - r.first) + w, kind, sl.stream));
      }
    count_copies(static_cast<size_t>(cnt) * runs.size());
    return RS_OK;
  }

  int send(Slot& sl, int cnt, size_t w) const {
    auto* h = static_cast<uint8_t*>(sl.host.p);
    auto* d = static_cast<uint8_t*>(sl.dev.p);
    auto* meta = static_cast<uint8_t*>(sl.meta.p);
    int* dstatus = reinterpret_cast<int*>(meta + ML.status_off);
    int rc;
    if ((rc = copy_rows(sl, in_runs, d, h, cnt, w, hipMemcpyHostToDevice))) return rc;
    if (verify) HIPCHK(hipMemsetAsync(dstatus, 0, sizeof(int) * cnt, sl.stream));
    if (verify) count_copies(2);  // the memset and the status words' D2H below
    HIPCHK(launch_groups(*tp, ML, cnt, meta, w, sl.stream, 1, sl.meta_hint));
    if (!out_runs.empty() && (rc = copy_rows(sl, out_runs, h, d, cnt, w, hipMemcpyDeviceToHost)))
      return rc;
    if (verify)
      HIPCHK(hipMemcpyAsync(sl.hstat.p, dstatus, sizeof(int) * cnt, hipMemcpyDeviceToHost,
                            sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    return RS_OK;
  }
};

// In-place kernels on host-coherent staging (rs_apply_small): the kernel reads the
// inputs and writes the outputs over PCIe, one dispatch per chunk and launch group, and
// the host spins on the kernel's completion flag. The staged transport spends three
// dependent dispatches (H2D, kernel, D2H) per chunk, which bound 4 KiB calls at ~29 us
// (DESIGN.md §7.4). Calls of at most CALLFS_RS_SMALL_MAX_BYTES of staging run as one
// chunk on slot 0; with CALLFS_RS_INPLACE_PIPELINE=1 (A/B) larger calls run the staged
// transport's chunks this way. Staging: [spc stripes][status words][completion flag],
// shards pitched to 16 B.
struct InplaceTransport {
  const std::shared_ptr<const Tables>& tp;
  const ChunkGeometry& g;
  const size_t stat_off, done_off;
  const bool verify;

  rs_ctx* const ctx;  // its copies counter

  InplaceTransport(rs_ctx* context, const std::shared_ptr<const Tables>& tables,
                   const ChunkGeometry& geo)
      : tp(tables), g(geo), stat_off(round_up(geo.spitch * geo.spc, 256)),
        done_off(round_up(stat_off + sizeof(int) * geo.spc, 256)),
        verify(!tables->check.empty()), ctx(context) {}

  // The v_perm tables and shard indices of every launch group uploaded to device memory
  // once per (slot, tables), and the finished-block counter of the completion flag.
  int prepare(Slot& sl) {
    int rc;
    if ((rc = sl.small.ensure(done_off + 256))) return rc;
    if (!sl.small_counter.p) {
      if ((rc = sl.small_counter.ensure(256))) return rc;
      HIPCHK(hipMemset(sl.small_counter.p, 0, 256));
    }
    if (sl.small_tables == tp) return RS_OK;
    const Tables& t = *tp;
    // per launch group: [v_perm tables][idx: 256 input + 16 row shard indices]
    std::vector<size_t> off;
    Packer pk;
    for (const Group& grp : t.groups) off.push_back(pk.take(grp.tabs.size() * sizeof(uint32_t) + 272));
    sl.small_tables = nullptr;
    if ((rc = sl.small_tabs.ensure(pk.off))) return rc;
    std::vector<uint8_t> h(pk.off, 0);
    for (size_t gi = 0; gi < t.groups.size(); ++gi) {
      const Group& grp = t.groups[gi];
      const size_t tb = grp.tabs.size() * sizeof(uint32_t);
      std::memcpy(h.data() + off[gi], grp.tabs.data(), tb);
      uint8_t* ix = h.data() + off[gi] + tb;
      for (int i = 0; i < t.k; ++i) ix[i] = static_cast<uint8_t>(t.valid[i]);
      for (size_t r = 0; r < grp.shard.size(); ++r) ix[256 + r] = static_cast<uint8_t>(grp.shard[r]);
    }
    HIPCHK(hipMemcpy(sl.small_tabs.p, h.data(), h.size(), hipMemcpyHostToDevice));
    ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
    sl.small_tables = tp;
    sl.small_tab_off = off;
    return RS_OK;
  }
  uint8_t* staging(Slot& sl) const { return static_cast<uint8_t*>(sl.small.p); }
  const int* status(Slot& sl) const { return reinterpret_cast<const int*>(staging(sl) + stat_off); }
  int wait(Slot& sl) const {
    const int* done = reinterpret_cast<const int*>(staging(sl) + done_off);
    // ~5 us sooner than the runtime's completion signal; past kSmallSpinUs the stream
    // wait, which also reports a faulted kernel
    if (!spin_until(done, sl.small_seq, kSmallSpinUs)) HIPCHK(hipStreamSynchronize(sl.stream));
    return RS_OK;
  }

  // One chunk in place: cnt stripes at base + b*spitch, shard i at + i*cpitch, w bytes per
  // shard; the last launch group releases the slot's sequence number into the completion
  // flag when all its blocks have finished.
  int send(Slot& sl, int cnt, size_t w) const {
    const Tables& t = *tp;
    uint8_t* base = staging(sl);
    int* st = reinterpret_cast<int*>(base + stat_off);
    int* done = reinterpret_cast<int*>(base + done_off);
    sl.small_seq = sl.small_seq >= 0x3fffffff ? 1 : sl.small_seq + 1;  // never 0
    // a fresh or moved buffer holds whatever it held: clear the flag before the launch
    __atomic_store_n(done, 0, __ATOMIC_RELEASE);
    if (verify) std::memset(st, 0, sizeof(int) * cnt);
    for (size_t gi = 0; gi < t.groups.size(); ++gi) {
      const Group& grp = t.groups[gi];
      SmallArgs A{};
      A.base = base;
      A.spitch = g.spitch;
      A.cpitch = g.cpitch;
      A.nvec = static_cast<uint32_t>((w + 15) / 16);
      A.S = static_cast<uint32_t>(w);
      A.K = t.k;
      A.R = static_cast<int>(grp.shard.size());
      A.batch = cnt;
      A.verify_mask = grp.verify_mask;
      const uint8_t* tb = static_cast<uint8_t*>(sl.small_tabs.p) + sl.small_tab_off[gi];
      A.tabs = reinterpret_cast<const uint32_t*>(tb);
      A.idx = tb + grp.tabs.size() * sizeof(uint32_t);
      for (int i = 0; i < std::min(t.k, 16); ++i)
        A.idx_in[i >> 2] |= static_cast<uint32_t>(t.valid[i]) << (8 * (i & 3));
      for (size_t r = 0; r < grp.shard.size(); ++r)
        A.idx_out[r >> 2] |= static_cast<uint32_t>(grp.shard[r]) << (8 * (r & 3));
      A.status = st;
      A.done = gi + 1 == t.groups.size() ? done : nullptr;
      A.counter = static_cast<unsigned*>(sl.small_counter.p);
      A.seq = sl.small_seq;
      HIPCHK(launch_small(A, sl.stream));
    }
    return RS_OK;
  }
};

template <class InF, class OutF>
int run_host_impl(rs_ctx* ctx, Lane& L, int device, const std::shared_ptr<const Tables>& tp,
                  size_t S, int batch, InF host_in, OutF host_out, int* stripe_status,
                  const Join* join, size_t col0) {
  HIPCHK(hipSetDevice(device));
  HostCall<InF, OutF> c{ctx, tp, S, batch, host_in, host_out, stripe_status, join, col0, tp->valid};
  c.ins.insert(c.ins.end(), tp->check.begin(), tp->check.end());
  if (direct_ok(c)) return run_direct(c, L.slot[0]);

  const size_t n = static_cast<size_t>(c.n());
  // the whole call as one in-place chunk on slot 0
  ChunkGeometry g;
  g.cpitch = round_up(S, 16);
  g.spitch = g.cpitch * n;
  if (g.spitch * static_cast<size_t>(batch) <= small_max_bytes() && batch <= 65535 &&
      S <= 0xFFFFFFF0u) {
    g.cw = S;
    g.spc = batch;
    g.ncol = g.nblk = 1;
    g.nslots = 1;
    InplaceTransport tr(ctx, tp, g);
    return run_chunks(c, L, g, tr);
  }
  g = chunk_geometry(S, static_cast<int>(n), batch, chunk_bytes(), pipeline_slots());
  if (inplace_pipeline() && g.cw <= 0xFFFFFFF0u && g.spc <= 65535) {
    g.cpitch = round_up(g.cw, 16);
    g.spitch = g.cpitch * n;
    InplaceTransport tr(ctx, tp, g);
    return run_chunks(c, L, g, tr);
  }
  StagedTransport tr(ctx, tp, g, c.ins);
  return run_chunks(c, L, g, tr);
}

template <class InF, class OutF>
int run_on(rs_ctx* ctx, Device* dev, const std::shared_ptr<const Tables>& tp, size_t S,
           int batch, InF host_in, OutF host_out, int* stripe_status,
           const Join* join = nullptr, size_t col0 = 0) {
  LaneGuard lg{ctx, dev, ctx->acquire(dev)};
  if (!lg.lane) return RS_E_HIP;
  const int rc =
      run_host_impl(ctx, *lg.lane, dev->id, tp, S, batch, host_in, host_out, stripe_status,
                    join, col0);
  if (rc != RS_OK && rc != RS_E_CORRUPT) {
    // never hand a lane with work in flight to the next caller
    for (Slot& sl : lg.lane->slot) {
      if (sl.stream) (void)hipStreamSynchronize(sl.stream);
      sl.pending = false;
    }
  }
  return rc;
}

// Ways to split one large object's columns over (device, lane) pairs (dispatch.hpp):
// objects of at least CALLFS_RS_SPLIT_MIN_BYTES over all n shards (default 256 MiB)
// are split CALLFS_RS_SPLIT_WAYS ways (default: one per device), each way on its own
// lane, so a multi-GPU host moves one object over every GPU's PCIe link at once.
int split_ways(const rs_ctx* ctx, size_t S, int n, int batch) {
  // read per call (cheap next to a >= 256 MiB object; tests change them in-process)
  const char* e = std::getenv("CALLFS_RS_SPLIT_MIN_BYTES");
  const unsigned long long min_bytes = e ? std::strtoull(e, nullptr, 0) : (256ull << 20);
  const char* w = std::getenv("CALLFS_RS_SPLIT_WAYS");
  const int ways_req = split_ways_request(w);  // unset: one per device; <= 1: no split
  return callfs::split_ways(ctx->devs.size(), kMaxLanesPerDevice, S, n, batch, min_bytes,
                            ways_req);
}

template <class InF, class OutF>
int run_host(rs_ctx* ctx, const std::shared_ptr<const Tables>& tp, size_t S, int batch,
             InF host_in, OutF host_out, int* stripe_status = nullptr,
             const Join* join = nullptr, bool count_call = true) {
  if (ctx->devs.empty()) return RS_E_HIP;
  if (count_call) ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  const size_t nd = ctx->devs.size();
  const unsigned base = ctx->rr.fetch_add(1);
  const int ways = split_ways(ctx, S, tp->k + tp->m, batch);
  if (ways == 1)
    return run_on(ctx, ctx->devs[device_slot(base, 0, nd)].get(), tp, S, batch, host_in,
                  host_out, stripe_status, join, 0);
  const std::vector<size_t> c = column_parts(S, ways);  // parts [c[p], c[p+1])
  std::vector<int> rc(ways, RS_OK), flag(ways, 0);
  std::vector<std::thread> th;
  for (int p = 0; p < ways; ++p)
    th.emplace_back([&, p] {
      const size_t c0 = c[p];
      if (c[p + 1] <= c0) return;
      rc[p] = run_on(ctx, ctx->devs[device_slot(base, p, nd)].get(), tp, c[p + 1] - c0, 1,
                     [&](int b, int i) { return host_in(b, i) + c0; },
                     [&](int b, int i) { return host_out(b, i) + c0; }, &flag[p], join, c0);
    });
  for (auto& t : th) t.join();
  int out = RS_OK;
  for (int p = 0; p < ways; ++p) {
    if (rc[p] != RS_OK && rc[p] != RS_E_CORRUPT) return rc[p];
    if (rc[p] == RS_E_CORRUPT) out = RS_E_CORRUPT;
  }
  if (out == RS_E_CORRUPT && stripe_status) stripe_status[0] = 1;
  return out;
}

// Single-stripe form used by the per-object entry points.
template <class InF, class OutF>
int run_host1(rs_ctx* ctx, const std::shared_ptr<const Tables>& tp, size_t S, InF in, OutF out,
              const Join* join = nullptr) {
  return run_host(ctx, tp, S, 1, [&](int, int i) { return in(i); },
                  [&](int, int i) { return out(i); }, nullptr, join);
}

// ---- the ragged pipeline -----------------------------------------------

// A batch call whose runnable stripes differ in shard size or erasure pattern runs as one
// pipeline over items (ragged_chunks.hpp) instead of one pipeline per (S, mask) group.
// CALLFS_RS_RAGGED_BATCH=0 keeps every call on the per-group path (A/B and fallback).
bool ragged_batch() {
  static const bool on = [] {
    const char* e = std::getenv("CALLFS_RS_RAGGED_BATCH");
    return !(e && *e == '0');
  }();
  return on;
}

// One ragged run: consecutive stripes of one class (ragged_classes) and segment
// (ragged_segments) with their pattern tables. Stripe s of the run is stripe ids[s] of the
// call's runnable list.
struct RaggedRun {
  rs_ctx* ctx;
  int k, m;
  MixedTables mt;
  RaggedShape sh;
  std::vector<int> ids;
  const Join* joins;  // nullable: one per runnable stripe of the call (codec-level batches)
  const Join* join_of(int id) const { return joins ? joins + id : nullptr; }
  const MixedPattern& pattern(int s) const { return mt.patterns[mt.pat[static_cast<size_t>(s)]]; }
  void count(size_t chunks, size_t copies) const {
    ctx->n_chunks.fetch_add(chunks, std::memory_order_relaxed);
    ctx->n_launches.fetch_add(chunks * mt.groups.size(), std::memory_order_relaxed);
    ctx->n_copies.fetch_add(copies, std::memory_order_relaxed);
  }
};

// What a lane's table cache is keyed by: the profile, the rows per pattern and the patterns.
std::string ragged_key(const RaggedRun& r) {
  std::string key = std::to_string(r.k) + "," + std::to_string(r.m) + "," + std::to_string(r.mt.rows) + ":";
  for (const MixedPattern& p : r.mt.patterns) key.append(reinterpret_cast<const char*>(p.mask.data()), p.mask.size());
  return key;
}

// The run's nibble-table arenas and compare masks in the lane's device buffer, per launch
// group [vmask][arena]; uploaded when the lane last held another run's.
struct RaggedDevTables {
  std::vector<size_t> vmask_off, arena_off;
};
int upload_ragged_tables(const RaggedRun& r, Lane& L, RaggedDevTables& dt) {
  Packer pk;
  for (const MixedGroup& g : r.mt.groups) {
    dt.vmask_off.push_back(pk.take(sizeof(uint32_t) * g.vmask.size()));
    dt.arena_off.push_back(pk.take(g.arena.size()));
  }
  std::string key = ragged_key(r);
  if (L.rag_tabs.p && L.rag_key == key) return RS_OK;
  L.rag_key.clear();
  if (const int rc = L.rag_tabs.ensure(pk.off)) return rc;
  std::vector<uint8_t> h(pk.off, 0);
  for (size_t gi = 0; gi < r.mt.groups.size(); ++gi) {
    const MixedGroup& g = r.mt.groups[gi];
    std::memcpy(h.data() + dt.vmask_off[gi], g.vmask.data(), sizeof(uint32_t) * g.vmask.size());
    std::memcpy(h.data() + dt.arena_off[gi], g.arena.data(), g.arena.size());
  }
  HIPCHK(hipMemcpy(L.rag_tabs.p, h.data(), h.size(), hipMemcpyHostToDevice));
  r.ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
  L.rag_key = std::move(key);
  return RS_OK;
}

// launch_ragged of every launch group over the chunk laid out by C at `base` (device-visible).
hipError_t launch_ragged_chunk(const RaggedRun& r, const ChunkLayout& C, uint8_t* base,
                               const uint8_t* tabs, const RaggedDevTables& dt, hipStream_t s) {
  for (size_t gi = 0; gi < r.mt.groups.size(); ++gi) {
    const MixedGroup& g = r.mt.groups[gi];
    ApplyArgs a{};
    a.in_tab = reinterpret_cast<const uint8_t* const*>(base + C.in_tab_off);
    a.out_tab = reinterpret_cast<uint8_t* const*>(base + C.out_tab_off[gi]);
    a.ltabs = tabs + dt.arena_off[gi];
    a.status = reinterpret_cast<int*>(base + C.status_off);
    a.status_stride = 1;
    a.K = r.k;
    a.R = g.R;
    a.batch = static_cast<int>(C.count);
    RaggedArgs x{};
    x.pat = reinterpret_cast<const uint32_t*>(base + C.pat_off);
    x.vmask = reinterpret_cast<const uint32_t*>(tabs + dt.vmask_off[gi]);
    x.size = reinterpret_cast<const uint64_t*>(base + C.size_off);
    x.tile0 = reinterpret_cast<const uint32_t*>(base + C.tile0_off);
    x.tile_stripe = reinterpret_cast<const uint32_t*>(base + C.tile_stripe_off);
    x.tab_stride = static_cast<uint32_t>(g.tab_stride);
    x.ntiles = C.ntiles;
    const hipError_t e = launch_ragged(a, x, C.any_tail, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Staged: one H2D of the chunk's input region (through the zeroed status words that open the
// output region), launch_ragged per launch group on the slot's device mirror, one D2H of the
// output region, then the slot's event.
struct RaggedStaged {
  const RaggedRun& r;
  Lane& L;
  RaggedDevTables dt;
  int prepare_run() { return upload_ragged_tables(r, L, dt); }
  int prepare(Slot& sl, size_t bytes) {
    int rc;
    if ((rc = sl.dev.ensure(bytes)) || (rc = sl.host.ensure(bytes))) return rc;
    return RS_OK;
  }
  uint8_t* staging(Slot& sl) const { return static_cast<uint8_t*>(sl.host.p); }
  uint8_t* base(Slot& sl) const { return static_cast<uint8_t*>(sl.dev.p); }
  int send(Slot& sl, const ChunkLayout& C) const {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const size_t head = C.status_off + sizeof(int) * C.count;
    HIPCHK(hipMemcpyAsync(d, h, head, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(launch_ragged_chunk(r, C, d, static_cast<const uint8_t*>(L.rag_tabs.p), dt, sl.stream));
    HIPCHK(hipMemcpyAsync(h + C.status_off, d + C.status_off, C.out_end - C.status_off,
                          hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.count(1, 2);
    return RS_OK;
  }
  int wait(Slot& sl) const {
    HIPCHK(hipEventSynchronize(sl.done));
    return RS_OK;
  }
};

// In place: rs_apply_small_ragged on host-coherent staging, one dispatch per launch group;
// the host spins on the completion flag the last group releases (as InplaceTransport). The
// pattern blocks ({compare mask, missing count}, v_perm tables; rs_kernels.hpp
// SmallRaggedArgs) live in the lane's device buffer, keyed like the arenas.
struct RaggedInplace {
  const RaggedRun& r;
  Lane& L;
  std::vector<size_t> tab_off;   // per launch group, bytes
  std::vector<uint32_t> pstride;  // per launch group, dwords
  size_t done_off = 0;

  int prepare_run() {
    const size_t P = r.mt.patterns.size();
    Packer pk;
    for (const MixedGroup& g : r.mt.groups) {
      pstride.push_back(4u + static_cast<uint32_t>(r.k) * g.R * kTabWords);
      tab_off.push_back(pk.take(sizeof(uint32_t) * pstride.back() * P));
    }
    std::string key = ragged_key(r);
    if (L.rag_small_tabs.p && L.rag_small_key == key) return RS_OK;
    L.rag_small_key.clear();
    if (const int rc = L.rag_small_tabs.ensure(pk.off)) return rc;
    std::vector<uint8_t> h(pk.off, 0);
    for (size_t gi = 0; gi < r.mt.groups.size(); ++gi) {
      const MixedGroup& g = r.mt.groups[gi];
      const size_t W = static_cast<size_t>(nibble_width(g.R));
      for (size_t p = 0; p < P; ++p) {
        auto* blk = reinterpret_cast<uint32_t*>(h.data() + tab_off[gi]) + p * pstride[gi];
        blk[0] = g.vmask[p];
        blk[1] = static_cast<uint32_t>(r.mt.patterns[p].missing);
        for (int i = 0; i < r.k; ++i)
          for (int row = 0; row < g.R; ++row) {
            // the coefficient is entry 1 of the low nibble table: c * 1
            const uint8_t c = g.arena[p * g.tab_stride + static_cast<size_t>(i) * 32u * W + W + row];
            perm_tables(c, blk + 4 + (static_cast<size_t>(i) * g.R + row) * kTabWords);
          }
      }
    }
    HIPCHK(hipMemcpy(L.rag_small_tabs.p, h.data(), h.size(), hipMemcpyHostToDevice));
    r.ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
    L.rag_small_key = std::move(key);
    return RS_OK;
  }
  int prepare(Slot& sl, size_t bytes) {
    done_off = round_up(bytes, 256);
    int rc;
    if ((rc = sl.small.ensure(done_off + 256))) return rc;
    if (!sl.small_counter.p) {
      if ((rc = sl.small_counter.ensure(256))) return rc;
      HIPCHK(hipMemset(sl.small_counter.p, 0, 256));
    }
    return RS_OK;
  }
  uint8_t* staging(Slot& sl) const { return static_cast<uint8_t*>(sl.small.p); }
  uint8_t* base(Slot& sl) const { return staging(sl); }
  int send(Slot& sl, const ChunkLayout& C) const {
    uint8_t* b = staging(sl);
    int* done = reinterpret_cast<int*>(b + done_off);
    sl.small_seq = sl.small_seq >= 0x3fffffff ? 1 : sl.small_seq + 1;  // never 0
    __atomic_store_n(done, 0, __ATOMIC_RELEASE);
    uint32_t max_nvec = 1;
    for (const ItemLayout& it : C.items) max_nvec = std::max(max_nvec, static_cast<uint32_t>(it.pitch / 16));
    for (size_t gi = 0; gi < r.mt.groups.size(); ++gi) {
      const MixedGroup& g = r.mt.groups[gi];
      SmallRaggedArgs A{};
      A.base = b;
      A.items = reinterpret_cast<const uint32_t*>(b + C.item_tab_off);
      A.ptabs = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(L.rag_small_tabs.p) + tab_off[gi]);
      A.pstride = pstride[gi];
      A.max_nvec = max_nvec;
      A.K = r.k;
      A.R = g.R;
      A.row0 = g.row0;
      A.nitems = static_cast<int>(C.count);
      A.status = reinterpret_cast<int*>(b + C.status_off);
      A.done = gi + 1 == r.mt.groups.size() ? done : nullptr;
      A.counter = static_cast<unsigned*>(sl.small_counter.p);
      A.seq = sl.small_seq;
      HIPCHK(launch_small_ragged(A, sl.stream));
    }
    r.count(1, 0);
    return RS_OK;
  }
  int wait(Slot& sl) const {
    const int* done = reinterpret_cast<const int*>(staging(sl) + done_off);
    if (!spin_until(done, sl.small_seq, kSmallSpinUs)) HIPCHK(hipStreamSynchronize(sl.stream));
    return RS_OK;
  }
  // what the kernel's 32-bit item table can address
  static bool fits(const ChunkLayout& C) {
    if (C.out_end >= (1ull << 35) || C.count > kRaggedMaxItems) return false;
    for (const ItemLayout& it : C.items)
      if (it.pitch > 0xFFFFFFF0u) return false;
    return true;
  }
};

// The chunk loop of a ragged run, in the style of run_chunks: chunks rotate through the
// lane's slots; per chunk the metadata is written and the input rows are copied into the
// slot's staging, the transport sends it, and the output rows of the chunk the slot held
// before are copied out first. in / out take a stripe of the call's runnable
// list and a shard index; flags (per runnable stripe) receive 1 where a compared row
// mismatched.
template <class Transport, class InF, class OutF>
int run_ragged_chunks(const RaggedRun& r, Lane& L, const std::vector<RaggedItem>& items,
                      const std::vector<ChunkLayout>& chunks, Transport& tr, InF& in, OutF& out,
                      int* flags) {
  int rc;
  if ((rc = tr.prepare_run())) return rc;
  size_t bytes = 0;
  for (const ChunkLayout& C : chunks) bytes = std::max(bytes, C.out_end);
  const size_t nchunks = chunks.size();
  const size_t nslots = std::min<size_t>(nchunks, static_cast<size_t>(pipeline_slots()));
  for (size_t si = 0; si < nslots; ++si) {
    if ((rc = tr.prepare(L.slot[si], bytes))) return rc;
    L.slot[si].pending = false;
  }
  const size_t k = static_cast<size_t>(r.k);
  std::vector<CopyPool::Seg> segs;
  auto drain = [&](Slot& sl) -> int {
    if (!sl.pending) return RS_OK;
    const int wrc = tr.wait(sl);
    if (wrc) return wrc;
    const ChunkLayout& C = chunks[sl.rag_chunk];
    uint8_t* h = tr.staging(sl);
    const int* st = reinterpret_cast<const int*>(h + C.status_off);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      if (st[j]) flags[id] = 1;
      const MixedPattern& pt = r.pattern(it.stripe);
      for (int row = 0; row < pt.missing; ++row) {
        const int i = pt.rows[static_cast<size_t>(row)];
        const auto tee = join_span(r.join_of(id), i, it.off, it.w);
        segs.push_back({out(id, i) + it.off,
                        h + C.items[j].out_off + C.items[j].pitch * static_cast<size_t>(row), it.w,
                        tee.first, tee.second});
      }
    }
    sl.pending = false;
    return RS_OK;
  };
  for (size_t c = 0; c < nchunks; ++c) {
    Slot& sl = L.slot[c % nslots];
    segs.clear();
    if ((rc = drain(sl))) return rc;
    // the last chunk's output rows leave before this chunk's layout overwrites them (chunks
    // of one run are laid out differently: its inputs may lie where those outputs were)
    if (!segs.empty()) r.ctx->pool.run(segs);
    segs.clear();
    const ChunkLayout& C = chunks[c];
    uint8_t* h = tr.staging(sl);
    uint8_t* b = tr.base(sl);
    // a row's address by the pattern's row number: written rows in the output part, compared
    // ones behind the k inputs
    auto row_at = [&](uint8_t* at, size_t j, int row) {
      const ItemLayout& il = C.items[j];
      const int missing = r.pattern(items[C.first + j].stripe).missing;
      return row < missing ? at + il.out_off + il.pitch * static_cast<size_t>(row)
                           : at + il.in_off + il.pitch * (k + static_cast<size_t>(row - missing));
    };
    fill_chunk_meta(C, r.sh, items, r.mt, r.mt.pat.data(), h,
                    [&](size_t j, int i) { return b + C.items[j].in_off + C.items[j].pitch * static_cast<size_t>(i); },
                    [&](size_t j, int row) { return row_at(b, j, row); });
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      const MixedPattern& pt = r.pattern(it.stripe);
      for (size_t i = 0; i < k; ++i) {
        const auto tee = join_span(r.join_of(id), pt.valid[i], it.off, it.w);
        segs.push_back({h + C.items[j].in_off + C.items[j].pitch * i, in(id, pt.valid[i]) + it.off, it.w,
                        tee.first, tee.second});
      }
      for (size_t row = static_cast<size_t>(pt.missing); row < pt.rows.size(); ++row)
        segs.push_back({row_at(h, j, static_cast<int>(row)), in(id, pt.rows[row]) + it.off, it.w});
    }
    r.ctx->pool.run(segs);
    if ((rc = tr.send(sl, C))) return rc;
    sl.pending = true;
    sl.rag_chunk = c;
  }
  for (size_t c = nchunks - nslots; c < nchunks; ++c) {
    segs.clear();
    if ((rc = drain(L.slot[c % nslots]))) return rc;
    r.ctx->pool.run(segs);
  }
  return RS_OK;
}

// Direct: every buffer of the run lies in rs_host_alloc memory. One metadata upload (the
// pointer tables name the caller's buffers), launch_ragged per launch group, the status
// words back, then a sync. No staging copies and no chunking; a codec-level batch's tees and
// joins are copy-pool work on the caller's bytes (present shards while the kernels run,
// rebuilt ones once they have landed), as in run_direct.
template <class InF, class OutF>
int run_ragged_direct(const RaggedRun& r, Lane& L, InF& in, OutF& out, int* flags) {
  std::vector<RaggedItem> items;
  uint64_t ntiles = 0;
  for (int s = 0; s < r.sh.stripes(); ++s) {
    items.push_back({s, 0, r.sh.size[static_cast<size_t>(s)]});
    ntiles += ragged_tiles(items.back().w);
  }
  if (ntiles > kRaggedMaxTiles) return RS_E_ARG;
  const ChunkLayout C = layout_chunk(r.sh, items, 0, items.size(), false);
  RaggedStaged tabs{r, L, {}};
  int rc;
  if ((rc = tabs.prepare_run())) return rc;
  Slot& sl = L.slot[0];
  if ((rc = sl.meta.ensure(C.out_end)) || (rc = sl.hmeta.ensure(C.out_end)) ||
      (rc = sl.hstat.ensure(sizeof(int) * C.count)))
    return rc;
  sl.meta_tables = nullptr;  // the uniform staged path refills its tables next time
  auto* h = static_cast<uint8_t*>(sl.hmeta.p);
  auto* d = static_cast<uint8_t*>(sl.meta.p);
  bool compares = false;
  auto shard = [&](size_t j, int i) -> uint8_t* {
    const int id = r.ids[j];
    const MixedPattern& pt = r.pattern(static_cast<int>(j));
    for (int row = 0; row < pt.missing; ++row)
      if (pt.rows[static_cast<size_t>(row)] == i) return out(id, i);
    return const_cast<uint8_t*>(in(id, i));
  };
  for (int s = 0; s < r.sh.stripes(); ++s) compares |= r.pattern(s).missing < r.mt.rows;
  fill_chunk_meta(C, r.sh, items, r.mt, r.mt.pat.data(), h,
                  [&](size_t j, int i) { return shard(j, r.pattern(static_cast<int>(j)).valid[static_cast<size_t>(i)]); },
                  [&](size_t j, int row) { return shard(j, r.pattern(static_cast<int>(j)).rows[static_cast<size_t>(row)]); });
  HIPCHK(hipMemcpyAsync(d, h, C.out_end, hipMemcpyHostToDevice, sl.stream));
  HIPCHK(launch_ragged_chunk(r, C, d, static_cast<const uint8_t*>(L.rag_tabs.p), tabs.dt, sl.stream));
  if (compares)
    HIPCHK(hipMemcpyAsync(sl.hstat.p, d + C.status_off, sizeof(int) * C.count, hipMemcpyDeviceToHost,
                          sl.stream));
  HIPCHK(hipEventRecord(sl.done, sl.stream));
  r.count(1, compares ? 2 : 1);
  auto join_segs = [&](bool present) {
    std::vector<CopyPool::Seg> js_segs;
    for (size_t j = 0; r.joins && j < C.count; ++j) {
      const int id = r.ids[j];
      const MixedPattern& pt = r.pattern(static_cast<int>(j));
      const size_t S = r.sh.size[j];
      if (present) {
        for (int i : pt.valid) {
          const auto js = join_span(r.join_of(id), i, 0, S);
          if (js.first) js_segs.push_back({js.first, in(id, i), js.second});
        }
      } else {
        for (int row = 0; row < pt.missing; ++row) {
          const int i = pt.rows[static_cast<size_t>(row)];
          const auto js = join_span(r.join_of(id), i, 0, S);
          if (js.first) js_segs.push_back({js.first, out(id, i), js.second});
        }
      }
    }
    r.ctx->pool.run(js_segs);
  };
  join_segs(true);
  HIPCHK(hipEventSynchronize(sl.done));
  join_segs(false);
  if (compares) {
    const int* st = static_cast<const int*>(sl.hstat.p);
    for (size_t j = 0; j < C.count; ++j)
      if (st[j]) flags[r.ids[j]] = 1;
  }
  return RS_OK;
}

// A heterogeneous batch call on one device and lane. The call's runnable stripes are listed
// by S[j] and present[j * n ..]; in(j, i) / out(j, i) give runnable stripe j's shard i.
// by_missing: a reconstruct without verification, whose stripes run in classes by missing
// count (a pattern's rows are its missing shards alone). flags[j] = 1 where stripe j's
// compared rows mismatched.
template <class InF, class OutF>
int run_ragged_impl(rs_ctx* ctx, Lane& L, int device, int k, int m, bool by_missing,
                    const std::vector<size_t>& S, const std::vector<uint8_t>& present, InF& in,
                    OutF& out, int* flags, const Join* joins) {
  HIPCHK(hipSetDevice(device));
  const int n = k + m, stripes = static_cast<int>(S.size());
  const size_t nn = static_cast<size_t>(n);
  // direct: every buffer pinned, and the call at or above the zero-copy threshold
  unsigned long long total = 0;
  for (size_t s : S) total += static_cast<unsigned long long>(s) * nn;
  bool direct = !ctx->pinned.empty() && total >= zero_copy_min(nn);
  for (int j = 0; direct && j < stripes; ++j)
    for (int i = 0; direct && i < n; ++i) {
      const bool written = !present[static_cast<size_t>(j) * nn + i];
      if (by_missing && !written) {
        // only the first k present shards are read
        int before = 0;
        for (int q = 0; q < i; ++q) before += present[static_cast<size_t>(j) * nn + q] != 0;
        if (before >= k) continue;
      }
      direct = ctx->pinned.contains(written ? out(j, i) : in(j, i), S[static_cast<size_t>(j)]);
    }
  for (int j = 0; direct && joins && j < stripes; ++j)
    direct = joins[j].len == 0 || ctx->pinned.contains(joins[j].out, joins[j].len);
  for (const RaggedClass& cls : ragged_classes(n, stripes, present.data(), by_missing)) {
    const int rows = by_missing ? cls.e : m;
    for (const auto& seg : ragged_segments(k, n, rows, cls.stripes, present.data(), kRaggedArenaBudget)) {
      RaggedRun r{ctx, k, m, {}, {}, {}, joins};
      r.ids.assign(cls.stripes.begin() + static_cast<ptrdiff_t>(seg.first),
                   cls.stripes.begin() + static_cast<ptrdiff_t>(seg.second));
      std::vector<uint8_t> pres(r.ids.size() * nn);
      for (size_t s = 0; s < r.ids.size(); ++s)
        std::memcpy(&pres[s * nn], &present[static_cast<size_t>(r.ids[s]) * nn], nn);
      const int count = static_cast<int>(r.ids.size());
      const MixedError me = by_missing ? build_mixed_tables_missing(k, m, rows, count, pres.data(), r.mt)
                                       : build_mixed_tables(k, m, count, pres.data(), r.mt);
      if (me == MixedError::kSingular) return RS_E_SINGULAR;
      if (me != MixedError::kOk) return RS_E_ARG;
      r.sh.k = k;
      for (const MixedGroup& g : r.mt.groups) r.sh.group_rows.push_back(g.R);
      for (int s = 0; s < count; ++s) {
        const MixedPattern& pt = r.pattern(s);
        r.sh.size.push_back(S[static_cast<size_t>(r.ids[static_cast<size_t>(s)])]);
        r.sh.nin.push_back(k + static_cast<int>(pt.rows.size()) - pt.missing);
        r.sh.nout.push_back(pt.missing);
      }
      int rc;
      if (direct) {
        if ((rc = run_ragged_direct(r, L, in, out, flags))) return rc;
        continue;
      }
      const std::vector<RaggedItem> items = ragged_items(r.sh, chunk_bytes());
      // the whole run as one in-place chunk on slot 0
      if (items.size() <= kRaggedMaxItems && small_max_bytes() > 0) {
        std::vector<ChunkLayout> one(1, layout_chunk(r.sh, items, 0, items.size()));
        if (one[0].out_end <= small_max_bytes() && RaggedInplace::fits(one[0])) {
          RaggedInplace tr{r, L, {}, {}, 0};
          if ((rc = run_ragged_chunks(r, L, items, one, tr, in, out, flags))) return rc;
          continue;
        }
      }
      const std::vector<ChunkLayout> chunks = ragged_chunks(r.sh, items, chunk_bytes());
      bool inplace = inplace_pipeline();
      for (const ChunkLayout& C : chunks) inplace = inplace && RaggedInplace::fits(C);
      for (const ChunkLayout& C : chunks)
        if (C.ntiles > kRaggedMaxTiles) return RS_E_ARG;
      if (inplace) {
        RaggedInplace tr{r, L, {}, {}, 0};
        rc = run_ragged_chunks(r, L, items, chunks, tr, in, out, flags);
      } else {
        RaggedStaged tr{r, L, {}};
        rc = run_ragged_chunks(r, L, items, chunks, tr, in, out, flags);
      }
      if (rc) return rc;
    }
  }
  return RS_OK;
}

template <class InF, class OutF>
int run_ragged(rs_ctx* ctx, int k, int m, bool by_missing, const std::vector<size_t>& S,
               const std::vector<uint8_t>& present, InF in, OutF out, int* flags,
               const Join* joins = nullptr) {
  if (ctx->devs.empty()) return RS_E_HIP;
  ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  ctx->n_ragged_calls.fetch_add(1, std::memory_order_relaxed);
  // one device and lane, chosen round-robin like any call (split_ways does not apply)
  Device* dev = ctx->devs[device_slot(ctx->rr.fetch_add(1), 0, ctx->devs.size())].get();
  LaneGuard lg{ctx, dev, ctx->acquire(dev)};
  if (!lg.lane) return RS_E_HIP;
  const int rc = run_ragged_impl(ctx, *lg.lane, dev->id, k, m, by_missing, S, present, in, out, flags, joins);
  if (rc != RS_OK) {
    // never hand a lane with work in flight to the next caller
    for (Slot& sl : lg.lane->slot) {
      if (sl.stream) (void)hipStreamSynchronize(sl.stream);
      sl.pending = false;
    }
  }
  return rc;
}

// The encode tables of RS(k, m): every data shard present, the parity rows computed.
std::shared_ptr<const Tables> encode_tables(rs_ctx* ctx, int k, int m) {
  uint8_t present[256];
  for (int i = 0; i < k + m; ++i) present[i] = i < k;
  return ctx->cache.get(k, m, present, false);
}

// Shared by rs_reconstruct / rs_codec_decode. verify=true fuses upstream Verify.
int reconstruct_host(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                     bool verify, Join* join = nullptr) {
  const int n = k + m;
  size_t S = 0;
  int np = 0;
  int rc = check_lens(n, lens, true, &S, &np);
  if (rc) return rc;
  if (np < k) return RS_E_TOO_FEW_SHARDS;
  if (np == n && !verify) return RS_OK;
  for (int i = 0; i < n; ++i)
    if (!shards[i]) return RS_E_ARG;
  uint8_t present[256];
  for (int i = 0; i < n; ++i) present[i] = lens[i] != 0;
  auto t = ctx->cache.get(k, m, present, verify);
  if (!t) return RS_E_SINGULAR;
  if (t->groups.empty()) return RS_OK;
  if (join) {
    join->S = S;
    join->len = std::min(join->len, S * k);
  }
  rc = run_host1(ctx, t, S, [&](int i) { return shards[i]; }, [&](int i) { return shards[i]; },
                 join);
  if (rc == RS_OK || rc == RS_E_CORRUPT) {
    for (int i : t->missing) lens[i] = S;
    if (join) join->done = true;
  }
  return rc;
}

int first_error(const int* status, int batch) {
  for (int b = 0; b < batch; ++b)
    if (status[b]) return status[b];
  return RS_OK;
}

// The runnable objects of a codec-level batch, routed as rs_encode_batch /
// rs_reconstruct_batch route their stripes: one (S, mask) group runs the uniform pipeline,
// two or more run one ragged pipeline (CALLFS_RS_RAGGED_BATCH=0: one pipeline per group).
// S, present (n flags each), joins and flags are indexed by object; in(b, i) / out(b, i)
// give object b's shard i. verify: the tables compare the present shards beyond the first k.
template <class InF, class OutF>
int run_codec_batch(rs_ctx* ctx, int k, int m, bool verify, const BatchGroups& groups,
                    const std::vector<size_t>& S, const std::vector<uint8_t>& present,
                    const std::vector<Join>& joins, InF in, OutF out, std::vector<int>& flags) {
  const size_t n = static_cast<size_t>(k + m);
  int rc;
  if (groups.by_key.size() >= 2 && ragged_batch()) {
    std::vector<int> ids;
    for (auto& kv : groups.by_key) ids.insert(ids.end(), kv.second.begin(), kv.second.end());
    std::sort(ids.begin(), ids.end());
    std::vector<size_t> Sj(ids.size());
    std::vector<uint8_t> pres(ids.size() * n);
    std::vector<Join> jj(ids.size());
    for (size_t j = 0; j < ids.size(); ++j) {
      const size_t b = static_cast<size_t>(ids[j]);
      Sj[j] = S[b];
      std::memcpy(&pres[j * n], &present[b * n], n);
      jj[j] = joins[b];
    }
    std::vector<int> fj(ids.size(), 0);
    rc = run_ragged(ctx, k, m, false, Sj, pres, [&](int j, int i) { return in(ids[j], i); },
                    [&](int j, int i) { return out(ids[j], i); }, fj.data(), jj.data());
    for (size_t j = 0; j < ids.size(); ++j) flags[static_cast<size_t>(ids[j])] = fj[j];
    return rc;
  }
  bool first = true;
  for (auto& kv : groups.by_key) {
    const std::vector<int>& ids = kv.second;
    auto t = ctx->cache.get(k, m, BatchGroups::present(kv.first), verify);
    if (!t) return RS_E_SINGULAR;
    std::vector<Join> jj;
    for (int b : ids) jj.push_back(joins[static_cast<size_t>(b)]);
    std::vector<int> fj(ids.size(), 0);
    rc = run_host(ctx, t, BatchGroups::shard_size(kv.first), static_cast<int>(ids.size()),
                  [&](int b, int i) { return in(ids[b], i); },
                  [&](int b, int i) { return out(ids[b], i); }, fj.data(), jj.data(), first);
    first = false;
    if (rc != RS_OK && rc != RS_E_CORRUPT) return rc;
    for (size_t j = 0; j < ids.size(); ++j) flags[static_cast<size_t>(ids[j])] = fj[j];
  }
  return RS_OK;
}

}  // namespace

// ---- exported: per-object calls ---------------------------------------------------------

extern "C" {

int rs_encode(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* const* data,
              uint8_t* const* parity) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !data || !parity) return RS_E_ARG;
  if (S == 0) return RS_E_NO_DATA;  // upstream Encode: checkShards -> ErrShardNoData
  auto t = encode_tables(ctx, k, m);
  if (!t) return RS_E_SINGULAR;
  return run_host1(ctx, t, S, [&](int i) { return data[i]; },
                  [&](int i) { return parity[i - k]; });
}

int rs_codec_encode(rs_ctx* ctx, int k, int m, const uint8_t* data, size_t len,
                    uint8_t* shards_out, size_t out_cap, size_t* shard_size) {
  DeviceGuard dg;
  // codec.go:22-24 profile check, :26 New, :31 Split, :36 Encode. Upstream New accepts
  // k+m > 256 (Leopard), so an empty object fails in Split before the profile is
  // found unsupported here.
  if (k < 1 || m < 1) return RS_E_INVALID_PROFILE;
  if (!ctx || !shard_size || (len && (!data || !shards_out))) return RS_E_ARG;
  if (len == 0) return RS_E_SHORT_DATA;
  int rc = check_profile(k, m);
  if (rc) return rc;
  const size_t S = (len + k - 1) / k;
  const int n = k + m;
  if (out_cap < S * n) return RS_E_ARG;
  auto t = encode_tables(ctx, k, m);
  if (!t) return RS_E_SINGULAR;
  *shard_size = S;
  const bool overlap = shards_out != data && shards_out < data + len && data < shards_out + S * n;
  if (shards_out == data || overlap) {
    if (overlap) std::memmove(shards_out, data, len);
    std::memset(shards_out + len, 0, S * k - len);  // Split zero padding
    return run_host1(ctx, t, S, [&](int i) { return shards_out + S * i; },
                    [&](int i) { return shards_out + S * i; });
  }
  // Disjoint buffers: the partial last shard and its zero padding go to shards_out first;
  // the full data shards are staged straight from `data`, and the staging copies tee
  // them into shards_out (no separate object-sized copy).
  const size_t full = len / S;
  std::memcpy(shards_out + full * S, data + full * S, len - full * S);
  std::memset(shards_out + len, 0, S * k - len);  // Split zero padding
  Join tee{shards_out, full * S, S, k};
  return run_host1(ctx, t, S,
                   [&](int i) {
                     return static_cast<size_t>(i) < full ? data + S * i : shards_out + S * i;
                   },
                   [&](int i) { return shards_out + S * i; }, &tee);
}

int rs_reconstruct(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens) return RS_E_ARG;
  return reconstruct_host(ctx, k, m, shards, lens, false);
}

int rs_verify(rs_ctx* ctx, int k, int m, const uint8_t* const* shards, const size_t* lens,
              int* ok) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens || !ok) return RS_E_ARG;
  const int n = k + m;
  size_t S = 0;
  int np = 0;
  if ((rc = check_lens(n, lens, false, &S, &np))) return rc;
  uint8_t present[256];
  for (int i = 0; i < n; ++i) present[i] = 1;
  auto t = ctx->cache.get(k, m, present, true);
  if (!t) return RS_E_SINGULAR;
  rc = run_host1(ctx, t, S, [&](int i) { return shards[i]; },
                 [&](int) { return static_cast<uint8_t*>(nullptr); });
  if (rc == RS_OK || rc == RS_E_CORRUPT) {
    *ok = rc == RS_OK;
    return RS_OK;
  }
  return rc;
}

int rs_codec_decode(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                    uint8_t* out, int64_t original_size) {
  DeviceGuard dg;
  // codec.go:46-48 profile, :50 New, :55 Reconstruct, :59-65 Verify, :67-77 join/trim
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens || original_size < 0 || (original_size && !out)) return RS_E_ARG;
  Join join{out, static_cast<size_t>(original_size), 0, k};
  rc = reconstruct_host(ctx, k, m, shards, lens, true, &join);
  if (rc) return rc;
  const size_t S = lens[0];
  if (static_cast<uint64_t>(S) * k < static_cast<uint64_t>(original_size))
    return RS_E_INSUFFICIENT;
  if (join.done) return RS_OK;  // joined on the way through the pipeline
  size_t left = static_cast<size_t>(original_size);
  std::vector<CopyPool::Seg> segs;
  for (int i = 0; i < k && left; ++i) {
    const size_t c = std::min(S, left);
    segs.push_back({out + S * i, shards[i], c});
    left -= c;
  }
  ctx->pool.run(segs);
  return RS_OK;
}

// ---- exported: batched host-memory calls ------------------------------------------------

int rs_encode_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                    const uint8_t* const* data, uint8_t* const* parity, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!sizes || !data || !parity || !status))) return RS_E_ARG;
  const int n = k + m;
  uint8_t present[256];
  for (int i = 0; i < n; ++i) present[i] = i < k;
  BatchGroups groups;
  for (int b = 0; b < batch; ++b) {
    status[b] = sizes[b] ? RS_OK : RS_E_NO_DATA;  // upstream Encode: ErrShardNoData
    if (sizes[b]) groups.add(sizes[b], present, n, b);
  }
  if (groups.by_key.size() >= 2 && ragged_batch()) {
    // two or more shard sizes: one ragged pipeline over the runnable stripes
    std::vector<int> ids;
    std::vector<size_t> S;
    for (int b = 0; b < batch; ++b)
      if (sizes[b]) {
        ids.push_back(b);
        S.push_back(sizes[b]);
      }
    std::vector<uint8_t> pres(ids.size() * n);
    for (size_t j = 0; j < ids.size(); ++j) std::memcpy(&pres[j * n], present, n);
    std::vector<int> flags(ids.size(), 0);
    rc = run_ragged(ctx, k, m, false, S, pres,
                    [&](int j, int i) { return data[static_cast<size_t>(ids[j]) * k + i]; },
                    [&](int j, int i) { return parity[static_cast<size_t>(ids[j]) * m + i - k]; },
                    flags.data());
    if (rc) return rc;
    return first_error(status, batch);
  }
  auto t = encode_tables(ctx, k, m);
  if (!t) return RS_E_SINGULAR;
  bool first = true;
  for (auto& kv : groups.by_key) {
    const std::vector<int>& ids = kv.second;
    const size_t S = BatchGroups::shard_size(kv.first);
    rc = run_host(ctx, t, S, static_cast<int>(ids.size()),
                  [&](int b, int i) { return data[static_cast<size_t>(ids[b]) * k + i]; },
                  [&](int b, int i) { return parity[static_cast<size_t>(ids[b]) * m + i - k]; },
                  nullptr, nullptr, first);
    first = false;
    if (rc) return rc;
  }
  return first_error(status, batch);
}

int rs_reconstruct_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                         size_t* lens, int verify, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!shards || !lens || !status))) return RS_E_ARG;
  const int n = k + m;
  BatchGroups groups;
  uint8_t present[256];
  for (int b = 0; b < batch; ++b) {
    uint8_t* const* sh = shards + static_cast<size_t>(b) * n;
    const size_t* ln = lens + static_cast<size_t>(b) * n;
    size_t S = 0;
    int np = 0;
    status[b] = check_lens(n, ln, true, &S, &np);
    if (status[b]) continue;
    if (np < k) {
      status[b] = RS_E_TOO_FEW_SHARDS;
      continue;
    }
    if (np == n && !verify) continue;
    bool ok = true;
    for (int i = 0; i < n; ++i) {
      ok &= sh[i] != nullptr;
      present[i] = ln[i] != 0;
    }
    if (!ok) {
      status[b] = RS_E_ARG;
      continue;
    }
    groups.add(S, present, n, b);
  }
  std::vector<int> flags;
  if (groups.by_key.size() >= 2 && ragged_batch()) {
    // two or more (S, mask) groups: one ragged pipeline over the runnable stripes
    std::vector<int> ids;
    for (auto& kv : groups.by_key) ids.insert(ids.end(), kv.second.begin(), kv.second.end());
    std::sort(ids.begin(), ids.end());
    std::vector<size_t> S(ids.size());
    std::vector<uint8_t> pres(ids.size() * n);
    for (size_t j = 0; j < ids.size(); ++j) {
      const size_t* ln = lens + static_cast<size_t>(ids[j]) * n;
      for (int i = 0; i < n; ++i) {
        pres[j * n + i] = ln[i] != 0;
        if (ln[i]) S[j] = ln[i];
      }
    }
    flags.assign(ids.size(), 0);
    auto sh = [&](int j, int i) { return shards[static_cast<size_t>(ids[j]) * n + i]; };
    rc = run_ragged(ctx, k, m, verify == 0, S, pres, sh, sh, flags.data());
    if (rc) return rc;
    for (size_t j = 0; j < ids.size(); ++j) {
      if (flags[j]) status[ids[j]] = RS_E_CORRUPT;
      for (int i = 0; i < n; ++i)
        if (!pres[j * n + i]) lens[static_cast<size_t>(ids[j]) * n + i] = S[j];
    }
    return first_error(status, batch);
  }
  bool first = true;
  for (auto& kv : groups.by_key) {
    const std::vector<int>& ids = kv.second;
    const size_t S = BatchGroups::shard_size(kv.first);
    auto t = ctx->cache.get(k, m, BatchGroups::present(kv.first), verify != 0);
    if (!t) return RS_E_SINGULAR;
    if (!t->groups.empty()) {
      flags.assign(ids.size(), 0);
      rc = run_host(ctx, t, S, static_cast<int>(ids.size()),
                    [&](int b, int i) { return shards[static_cast<size_t>(ids[b]) * n + i]; },
                    [&](int b, int i) { return shards[static_cast<size_t>(ids[b]) * n + i]; },
                    flags.data(), nullptr, first);
      first = false;
      if (rc != RS_OK && rc != RS_E_CORRUPT) return rc;
      for (size_t j = 0; j < ids.size(); ++j)
        if (flags[j]) status[ids[j]] = RS_E_CORRUPT;
    }
    for (int b : ids)
      for (int i : t->missing) lens[static_cast<size_t>(b) * n + i] = S;
  }
  return first_error(status, batch);
}

// ---- exported: codec-level batches (objects in, objects out) ----------------------------

int rs_codec_encode_batch(rs_ctx* ctx, int k, int m, int batch, const uint8_t* const* data,
                          const size_t* lens, uint8_t* const* shards_out, const size_t* out_caps,
                          size_t* shard_sizes, int* status) {
  DeviceGuard dg;
  // per object codec.go:31 Split and :36 Encode; the profile (:22-26) is the call's
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 ||
      (batch && (!data || !lens || !shards_out || !out_caps || !shard_sizes || !status)))
    return RS_E_ARG;
  const int n = k + m;
  const size_t B = static_cast<size_t>(batch);
  std::vector<uint8_t> present(B * n, 0);
  std::vector<SplitPlan> plan(B);
  std::vector<size_t> S(B, 0);
  std::vector<Join> tees(B, Join{nullptr, 0, 0, k});
  BatchGroups groups;
  for (size_t b = 0; b < B; ++b) {
    if (lens[b] == 0) {
      status[b] = RS_E_SHORT_DATA;  // upstream Split
      continue;
    }
    plan[b] = split_plan(k, lens[b]);
    if (!data[b] || !shards_out[b] || out_caps[b] / static_cast<size_t>(n) < plan[b].S) {
      status[b] = RS_E_ARG;
      continue;
    }
    status[b] = RS_OK;
    shard_sizes[b] = S[b] = plan[b].S;
    split_prepare(plan[b], n, data[b], shards_out[b]);
    tees[b] = split_tee(plan[b], shards_out[b]);
    for (int i = 0; i < k; ++i) present[b * n + i] = 1;
    groups.add(S[b], &present[b * n], n, static_cast<int>(b));
  }
  std::vector<int> flags(B, 0);
  rc = run_codec_batch(ctx, k, m, false, groups, S, present, tees,
                       [&](int b, int i) { return split_row(plan[b], data[b], shards_out[b], i); },
                       [&](int b, int i) { return shards_out[b] + S[b] * static_cast<size_t>(i); },
                       flags);
  if (rc) return rc;
  return first_error(status, batch);
}

int rs_codec_decode_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                          size_t* lens, uint8_t* const* out, const int64_t* original_sizes,
                          int* status) {
  DeviceGuard dg;
  // per object codec.go:55 Reconstruct, :59-65 Verify, :67-77 join / trim
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!shards || !lens || !out || !original_sizes || !status)))
    return RS_E_ARG;
  const int n = k + m;
  const size_t B = static_cast<size_t>(batch);
  std::vector<uint8_t> present(B * n, 0);
  std::vector<size_t> S(B, 0);
  std::vector<Join> joins(B, Join{nullptr, 0, 0, k});
  BatchGroups groups;
  for (size_t b = 0; b < B; ++b) {
    uint8_t* const* sh = shards + b * n;
    const size_t* ln = lens + b * n;
    int np = 0;
    if ((status[b] = check_lens(n, ln, true, &S[b], &np))) continue;
    if (np < k) {
      status[b] = RS_E_TOO_FEW_SHARDS;
      continue;
    }
    bool ok = original_sizes[b] >= 0 && (original_sizes[b] == 0 || out[b]);
    for (int i = 0; i < n; ++i) ok &= sh[i] != nullptr;
    if (!ok) {
      status[b] = RS_E_ARG;
      continue;
    }
    for (int i = 0; i < n; ++i) present[b * n + i] = ln[i] != 0;
    joins[b] = decode_join(k, S[b], out[b], static_cast<size_t>(original_sizes[b]));
    groups.add(S[b], &present[b * n], n, static_cast<int>(b));
  }
  std::vector<int> flags(B, 0);
  auto shard = [&](int b, int i) { return shards[static_cast<size_t>(b) * n + i]; };
  rc = run_codec_batch(ctx, k, m, true, groups, S, present, joins, shard, shard, flags);
  if (rc) return rc;
  for (auto& kv : groups.by_key)
    for (int b : kv.second) {
      for (int i = 0; i < n; ++i)
        if (!present[static_cast<size_t>(b) * n + i]) lens[static_cast<size_t>(b) * n + i] = S[b];
      if (flags[b])
        status[b] = RS_E_CORRUPT;
      else if (static_cast<uint64_t>(S[b]) * k < static_cast<uint64_t>(original_sizes[b]))
        status[b] = RS_E_INSUFFICIENT;
    }
  return first_error(status, batch);
}

}  // extern "C"
