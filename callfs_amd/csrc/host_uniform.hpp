// The uniform pipeline of the host-memory path: one call over `batch` stripes that share one
// table set and one shard size (HostCall). It owns the zero-copy launches on the caller's
// rs_host_alloc buffers (run_direct), the chunk loop over a lane's slots (run_chunks), the two
// transports that send a chunk to the GPU and await it -- staged (H2D / kernels / D2H) or in
// place on host-coherent staging (one dispatch per launch group) -- and run_host, which
// picks the device, the lane and the column split of one call. Included by rs_host.cpp only.
#pragma once

#include "host_common.hpp"

namespace callfs {
namespace {

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
  std::vector<CopyPool::Seg> present, rebuilt;
  for (int b = 0; c.join && b < batch; ++b)
    for (int i = 0; i < t.k; ++i) {
      const auto js = join_span(c.join_of(b), i, c.col0, c.S);
      if (!js.first) continue;
      if (is_out[i]) rebuilt.push_back({js.first, c.out(b, i), js.second});
      else present.push_back({js.first, c.in(b, i), js.second});
    }
  if ((rc = join_around_launch(c.ctx, sl, present, rebuilt))) return rc;
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
// the host spins on the kernel's completion flag (host_common.hpp). The staged transport
// spends three dependent dispatches (H2D, kernel, D2H) per chunk, which bound 4 KiB calls at
// ~29 us. Calls of at most CALLFS_RS_SMALL_MAX_BYTES of staging run as one
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

  // The slot's staging and completion flag, and the v_perm tables and shard indices of
  // every launch group uploaded to device memory once per (slot, tables).
  int prepare(Slot& sl) {
    int rc;
    if ((rc = done_flag_ensure(sl, done_off))) return rc;
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
  int wait(Slot& sl) const { return done_flag_wait(sl, done_off); }

  // One chunk in place: cnt stripes at base + b*spitch, shard i at + i*cpitch, w bytes per
  // shard; the last launch group releases the slot's sequence number into the completion
  // flag when all its blocks have finished.
  int send(Slot& sl, int cnt, size_t w) const {
    const Tables& t = *tp;
    uint8_t* base = staging(sl);
    int* st = reinterpret_cast<int*>(base + stat_off);
    int* done = done_flag_arm(sl, done_off);
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

// One call on one lane: zero-copy, one in-place chunk, or the chunk pipeline.
template <class InF, class OutF>
int run_on_lane(rs_ctx* ctx, Lane& L, int device, const std::shared_ptr<const Tables>& tp,
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
  return with_lane(ctx, dev, [&](Lane& L) {
    return run_on_lane(ctx, L, dev->id, tp, S, batch, host_in, host_out, stripe_status, join, col0);
  });
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

}  // namespace
}  // namespace callfs
