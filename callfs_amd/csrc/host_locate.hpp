// Locate on host memory: rs_locate, rs_locate_batch and the locate step of
// rs_heal_batch are one route, the ragged pipeline of §7.5 on its staged transport. The
// stripes with a compared shard become items (ragged_chunks.hpp: whole stripes, or column
// parts of stripes too large for a chunk); a chunk stages its items' k read shards and r'
// compared shards as input rows, moves with one H2D (rows, metadata, zeroed status words and
// counts), runs launch_locate on the slot's device mirror and brings the status words and the
// counts back with one D2H. Counts are additive over byte columns, so a part's counts are added
// into its stripe's on the host. Included by rs_host.cpp only.
#pragma once

#include "host_common.hpp"
#include "locate_tables.hpp"
#include "ragged_chunks.hpp"

namespace callfs {
namespace {

// One run: consecutive stripes whose pattern tables fit kRaggedArenaBudget. Stripe s of the run
// is stripe ids[s] of the call.
struct LocateRun {
  rs_ctx* ctx;
  int k, m;
  LocateTables t;
  RaggedShape sh;  // nin = k + r', nout = 0
  std::vector<int> ids;
  bool correct = false;  // launch_correct in launch_locate's place (host_correct.hpp)
  const MixedTables& mt() const { return t.ragged.mixed; }
  size_t bins() const { return static_cast<size_t>(k + m) + 1; }
};

// The run's tables in the lane's device buffer: [vmask][nrows][arena][gf][loc]; uploaded when
// the lane last held other tables (the ragged runs' keys start with a digit, the update runs'
// with 'U').
struct LocateDevTables {
  size_t vmask_off = 0, nrows_off = 0, arena_off = 0, gf_off = 0, loc_off = 0;
};
int upload_locate_tables(const LocateRun& r, Lane& L, LocateDevTables& dt) {
  const MixedGroup& g = r.mt().groups[0];
  Packer pk;
  dt.vmask_off = pk.take(sizeof(uint32_t) * g.vmask.size());
  dt.nrows_off = pk.take(sizeof(uint32_t) * g.nrows.size());
  dt.arena_off = pk.take(g.arena.size());
  dt.gf_off = pk.take(r.t.gf.size());
  dt.loc_off = pk.take(r.t.loc.size());
  // ("L": single plans' tables, "M": pair plans')
  std::string key = (r.t.max_errors > 1 ? "M" : "L") + std::to_string(r.k) + "," + std::to_string(r.m) + ":";
  for (const MixedPattern& p : r.mt().patterns) key.append(reinterpret_cast<const char*>(p.mask.data()), p.mask.size());
  if (L.rag_tabs.p && L.rag_key == key) return RS_OK;
  L.rag_key.clear();
  if (const int rc = L.rag_tabs.ensure(pk.off)) return rc;
  std::vector<uint8_t> h(pk.off, 0);
  std::memcpy(h.data() + dt.vmask_off, g.vmask.data(), sizeof(uint32_t) * g.vmask.size());
  std::memcpy(h.data() + dt.nrows_off, g.nrows.data(), sizeof(uint32_t) * g.nrows.size());
  std::memcpy(h.data() + dt.arena_off, g.arena.data(), g.arena.size());
  std::memcpy(h.data() + dt.gf_off, r.t.gf.data(), r.t.gf.size());
  std::memcpy(h.data() + dt.loc_off, r.t.loc.data(), r.t.loc.size());
  HIPCHK(hipMemcpy(L.rag_tabs.p, h.data(), h.size(), hipMemcpyHostToDevice));
  r.ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
  L.rag_key = std::move(key);
  return RS_OK;
}

// A chunk's counts lie behind its layout: count * (k + m + 1) words, zeroed on the way in.
inline size_t locate_counts_off(const ChunkLayout& C) { return round_up(C.out_end, 256); }
inline size_t locate_chunk_bytes(const LocateRun& r, const ChunkLayout& C) {
  return locate_counts_off(C) + sizeof(uint64_t) * C.count * r.bins();
}

// The chunk loop, in the style of run_update_chunks. shard_of takes a stripe of the call and a
// shard index; counts (the call's, batch * (k + m + 1)) are added into and flags[b] set where a
// compared row of stripe b mismatched. back(r, C, items, d, cn) runs once a chunk's counts `cn`
// are on the host and its device rows at `d` still stand (LocateNoBack: nothing to do).
struct LocateNoBack {
  int operator()(const LocateRun&, const ChunkLayout&, const std::vector<RaggedItem>&, const uint8_t*,
                 const uint64_t*) const {
    return RS_OK;
  }
};
template <class ShardF, class BackF>
int run_locate_chunks(const LocateRun& r, Lane& L, const std::vector<RaggedItem>& items,
                      const std::vector<ChunkLayout>& chunks, ShardF& shard_of, uint64_t* counts,
                      int* flags, BackF& back) {
  int rc;
  LocateDevTables dt;
  if ((rc = upload_locate_tables(r, L, dt))) return rc;
  size_t bytes = 0;
  for (const ChunkLayout& C : chunks) bytes = std::max(bytes, locate_chunk_bytes(r, C));
  const size_t nchunks = chunks.size();
  const size_t nslots = std::min<size_t>(nchunks, static_cast<size_t>(pipeline_slots()));
  for (size_t si = 0; si < nslots; ++si) {
    Slot& sl = L.slot[si];
    if ((rc = sl.dev.ensure(bytes)) || (rc = sl.host.ensure(bytes))) return rc;
    sl.pending = false;
  }
  const uint8_t* tabs = static_cast<const uint8_t*>(L.rag_tabs.p);
  const size_t k = static_cast<size_t>(r.k), nb = r.bins();
  const MixedGroup& g = r.mt().groups[0];
  auto drain = [&](Slot& sl) -> int {
    if (!sl.pending) return RS_OK;
    HIPCHK(hipEventSynchronize(sl.done));
    const ChunkLayout& C = chunks[sl.rag_chunk];
    const uint8_t* h = static_cast<const uint8_t*>(sl.host.p);
    const int* st = reinterpret_cast<const int*>(h + C.status_off);
    const uint64_t* cn = reinterpret_cast<const uint64_t*>(h + locate_counts_off(C));
    for (size_t j = 0; j < C.count; ++j) {
      const int id = r.ids[static_cast<size_t>(items[C.first + j].stripe)];
      if (st[j]) flags[id] = 1;
      for (size_t q = 0; q < nb; ++q) counts[static_cast<size_t>(id) * nb + q] += cn[j * nb + q];
    }
    sl.pending = false;
    return back(r, C, items, static_cast<const uint8_t*>(sl.dev.p), cn);
  };
  std::vector<CopyPool::Seg> segs;
  for (size_t c = 0; c < nchunks; ++c) {
    Slot& sl = L.slot[c % nslots];
    if ((rc = drain(sl))) return rc;
    const ChunkLayout& C = chunks[c];
    uint8_t* h = static_cast<uint8_t*>(sl.host.p);
    uint8_t* d = static_cast<uint8_t*>(sl.dev.p);
    // input row i of an item is its pattern's valid[i], row k + x its compared shard x; the
    // slots of out_tab past the item's r' hold null
    fill_chunk_meta(C, r.sh, items, r.mt(), r.mt().pat.data(), h,
                    [&](size_t j, int i) { return d + C.items[j].in_off + C.items[j].pitch * static_cast<size_t>(i); },
                    [&](size_t j, int row) -> uint8_t* {
                      const size_t rows = r.t.rows(r.mt().pat[static_cast<size_t>(items[C.first + j].stripe)]);
                      return static_cast<size_t>(row) < rows
                                 ? d + C.items[j].in_off + C.items[j].pitch * (k + static_cast<size_t>(row))
                                 : nullptr;
                    });
    const size_t total = locate_chunk_bytes(r, C);
    std::memset(h + C.status_off, 0, total - C.status_off);
    segs.clear();
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      const MixedPattern& pt = r.mt().patterns[r.mt().pat[static_cast<size_t>(it.stripe)]];
      const size_t rows = r.t.rows(r.mt().pat[static_cast<size_t>(it.stripe)]);
      for (size_t i = 0; i < k; ++i)
        segs.push_back({h + il.in_off + il.pitch * i, shard_of(id, pt.valid[i]) + it.off, it.w});
      for (size_t x = 0; x < rows; ++x)
        segs.push_back({h + il.in_off + il.pitch * (k + x), shard_of(id, pt.rows[x]) + it.off, it.w});
    }
    r.ctx->pool.run(segs);
    HIPCHK(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, sl.stream));
    ApplyArgs a{};
    a.in_tab = reinterpret_cast<const uint8_t* const*>(d + C.in_tab_off);
    a.out_tab = reinterpret_cast<uint8_t* const*>(d + C.out_tab_off[0]);
    a.ltabs = tabs + dt.arena_off;
    a.status = reinterpret_cast<int*>(d + C.status_off);
    a.status_stride = 1;
    a.K = r.k;
    a.R = g.R;
    a.batch = static_cast<int>(C.count);
    LocateArgs x{};
    x.r.pat = reinterpret_cast<const uint32_t*>(d + C.pat_off);
    x.r.vmask = reinterpret_cast<const uint32_t*>(tabs + dt.vmask_off);
    x.r.size = reinterpret_cast<const uint64_t*>(d + C.size_off);
    x.r.tile0 = reinterpret_cast<const uint32_t*>(d + C.tile0_off);
    x.r.tile_stripe = reinterpret_cast<const uint32_t*>(d + C.tile_stripe_off);
    x.r.tab_stride = static_cast<uint32_t>(g.tab_stride);
    x.r.ntiles = C.ntiles;
    x.nrows = reinterpret_cast<const uint32_t*>(tabs + dt.nrows_off);
    x.gf = tabs + dt.gf_off;
    x.loc = tabs + dt.loc_off;
    x.counts = reinterpret_cast<uint64_t*>(d + locate_counts_off(C));
    x.loc_stride = static_cast<uint32_t>(r.t.stride);
    x.nbins = static_cast<uint32_t>(nb);
    HIPCHK(r.correct ? launch_correct(a, x, C.any_tail, sl.stream)
                     : launch_locate(a, x, C.any_tail, sl.stream, {}, r.t.max_errors));
    HIPCHK(hipMemcpyAsync(h + C.status_off, d + C.status_off, total - C.status_off, hipMemcpyDeviceToHost,
                          sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_launches.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_copies.fetch_add(2, std::memory_order_relaxed);
    sl.pending = true;
    sl.rag_chunk = c;
  }
  for (size_t c = nchunks - nslots; c < nchunks; ++c)
    if ((rc = drain(L.slot[c % nslots]))) return rc;
  return RS_OK;
}

// The call's runnable stripes `ids` (each has more than k present shards, a nonzero size and
// its pointers) on one device and lane. sizes and present (0 / 1 flags, batch * (k + m)) are
// the whole call's; counts too, zeroed by the caller. max_errors 1 or 2 (2: pair tables and the
// pair kernel). correct (with max_errors 1): launch_correct, and `back`
// after every chunk (host_correct.hpp).
template <class ShardF, class BackF = LocateNoBack>
int run_locate(rs_ctx* ctx, int k, int m, int max_errors, const std::vector<int>& ids, const size_t* sizes,
               const uint8_t* present, ShardF shard_of, uint64_t* counts, int* flags, bool correct = false,
               BackF back = BackF()) {
  if (ids.empty()) return RS_OK;
  if (ctx->devs.empty()) return RS_E_HIP;
  ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  ctx->n_ragged_calls.fetch_add(1, std::memory_order_relaxed);
  Device* dev = ctx->devs[device_slot(ctx->rr.fetch_add(1), 0, ctx->devs.size())].get();
  const size_t n = static_cast<size_t>(k + m);
  return with_lane(ctx, dev, [&](Lane& L) -> int {
    HIPCHK(hipSetDevice(dev->id));
    const size_t per = pattern_arena_bytes(k, kLocateRows) + locate_stride(k, max_errors);
    const size_t max_patterns = std::max<size_t>(1, kRaggedArenaBudget / per);
    size_t begin = 0;
    while (begin < ids.size()) {
      std::set<std::string> seen;
      size_t end = begin;
      for (; end < ids.size(); ++end) {
        std::string key(reinterpret_cast<const char*>(present + static_cast<size_t>(ids[end]) * n), n);
        if (!seen.count(key) && seen.size() == max_patterns) break;
        seen.insert(std::move(key));
      }
      LocateRun r{ctx, k, m, {}, {}, {}, correct};
      r.ids.assign(ids.begin() + static_cast<ptrdiff_t>(begin), ids.begin() + static_cast<ptrdiff_t>(end));
      const int count = static_cast<int>(r.ids.size());
      std::vector<size_t> sz(r.ids.size());
      std::vector<uint8_t> pres(r.ids.size() * n);
      for (size_t s = 0; s < r.ids.size(); ++s) {
        sz[s] = sizes[r.ids[s]];
        std::memcpy(&pres[s * n], present + static_cast<size_t>(r.ids[s]) * n, n);
      }
      const TableError te = build_locate_tables(k, m, count, sz.data(), pres.data(), r.t, max_errors);
      if (te == TableError::kSingular) return RS_E_SINGULAR;
      if (te != TableError::kOk || r.mt().groups.size() != 1) return RS_E_ARG;
      r.sh.k = k;
      r.sh.group_rows.push_back(r.mt().groups[0].R);
      for (int s = 0; s < count; ++s) {
        r.sh.size.push_back(sz[static_cast<size_t>(s)]);
        r.sh.nin.push_back(k + static_cast<int>(r.t.rows(r.mt().pat[static_cast<size_t>(s)])));
        r.sh.nout.push_back(0);
      }
      const std::vector<RaggedItem> items = ragged_items(r.sh, chunk_bytes());
      const std::vector<ChunkLayout> chunks = ragged_chunks(r.sh, items, chunk_bytes());
      for (const ChunkLayout& C : chunks)
        if (C.ntiles > kRaggedMaxTiles) return RS_E_ARG;
      if (const int rc = run_locate_chunks(r, L, items, chunks, shard_of, counts, flags, back)) return rc;
      begin = end;
    }
    return RS_OK;
  });
}

}  // namespace
}  // namespace callfs
