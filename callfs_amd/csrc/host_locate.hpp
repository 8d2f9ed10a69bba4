// Locate and correct on host memory: rs_locate, rs_locate_batch, the
// locate step of rs_heal_batch and the correct calls (host_correct.hpp) are one route, a job of
// the chunk pipeline of §7.5 (host_chunks.hpp) on the staged transport's slots. The stripes
// with a compared shard become items (ragged_chunks.hpp: whole stripes, or column parts of
// stripes too large for a chunk); a chunk stages its items' k read shards and r' compared shards
// as input rows, moves with one H2D (rows, metadata, zeroed status words and counts), runs
// launch_locate -- a correct run: launch_correct -- on the slot's device mirror and brings the
// status words and the counts back with one D2H. Counts are additive over byte columns, so a
// part's counts are added into its stripe's on the host. A correct run then copies the rows its
// launch changed, those with a nonzero count, from the device mirror into the caller's shards,
// one D2H each; a chunk of clean stripes copies no shard byte back. Included by rs_host.cpp only.
#pragma once

#include "host_chunks.hpp"
#include "locate_tables.hpp"

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
  uint8_t* const* repair = nullptr;  // a correct run: the call's shards, batch * (k + m)
  const MixedTables& mt() const { return t.ragged.mixed; }
  size_t bins() const { return static_cast<size_t>(k + m) + 1; }
};

// A chunk's counts lie behind its layout: count * (k + m + 1) words, zeroed on the way in.
inline size_t locate_counts_off(const ChunkLayout& C) { return round_up(C.out_end, 256); }

// The route's job. shard_of takes a stripe of the call and a shard index; counts (the call's,
// batch * (k + m + 1)) are added into and flags[b] set where a compared row of stripe b
// mismatched.
template <class ShardF>
struct LocateJob : StagedSlots {
  const LocateRun& r;
  Lane& L;
  const std::vector<RaggedItem>& items;
  ShardF& shard_of;
  uint64_t* counts;
  int* flags;
  std::vector<size_t> tab_off;  // in the lane's device buffer: [vmask][nrows][arena][gf][loc]
  LocateJob(const LocateRun& run, Lane& lane, const std::vector<RaggedItem>& its, ShardF& sh, uint64_t* cn, int* fl)
      : r(run), L(lane), items(its), shard_of(sh), counts(cn), flags(fl) {}

  // (the ragged runs' keys start with a digit, the update runs' with 'U'; "L": single plans'
  // tables, "M": pair plans')
  int prepare_run() {
    const MixedGroup& g = r.mt().groups[0];
    const std::vector<TablePiece> pieces{{g.vmask.data(), sizeof(uint32_t) * g.vmask.size()},
                                         {g.nrows.data(), sizeof(uint32_t) * g.nrows.size()},
                                         {g.arena.data(), g.arena.size()},
                                         {r.t.gf.data(), r.t.gf.size()},
                                         {r.t.loc.data(), r.t.loc.size()}};
    std::string key = (r.t.max_errors > 1 ? "M" : "L") + std::to_string(r.k) + "," + std::to_string(r.m) + ":";
    for (const MixedPattern& p : r.mt().patterns) key.append(reinterpret_cast<const char*>(p.mask.data()), p.mask.size());
    return upload_lane_tables(r.ctx, L.rag_tabs, L.rag_key, std::move(key), pieces, tab_off);
  }
  size_t staging_bytes(const ChunkLayout& C) const { return locate_counts_off(C) + sizeof(uint64_t) * C.count * r.bins(); }
  uint32_t pattern(const ChunkLayout& C, size_t j) const { return r.mt().pat[static_cast<size_t>(items[C.first + j].stripe)]; }

  // Input row i of an item is its pattern's valid[i], row k + x its compared shard x; the slots
  // of out_tab past the item's r' hold null.
  int stage(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const size_t k = static_cast<size_t>(r.k);
    fill_chunk_meta(C, r.sh, items, r.mt(), r.mt().pat.data(), h,
                    [&](size_t j, int i) { return d + C.items[j].in_off + C.items[j].pitch * static_cast<size_t>(i); },
                    [&](size_t j, int row) -> uint8_t* {
                      return static_cast<size_t>(row) < r.t.rows(pattern(C, j))
                                 ? d + C.items[j].in_off + C.items[j].pitch * (k + static_cast<size_t>(row))
                                 : nullptr;
                    });
    std::memset(h + C.status_off, 0, staging_bytes(C) - C.status_off);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      const MixedPattern& pt = r.mt().patterns[pattern(C, j)];
      for (size_t i = 0; i < k; ++i)
        segs.push_back({h + il.in_off + il.pitch * i, shard_of(id, pt.valid[i]) + it.off, it.w});
      for (size_t x = 0; x < r.t.rows(pattern(C, j)); ++x)
        segs.push_back({h + il.in_off + il.pitch * (k + x), shard_of(id, pt.rows[x]) + it.off, it.w});
    }
    return RS_OK;
  }

  // One H2D of the whole chunk, the launch, one D2H from the status words on.
  int send(Slot& sl, const ChunkLayout& C) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const uint8_t* tabs = static_cast<const uint8_t*>(L.rag_tabs.p);
    const MixedGroup& g = r.mt().groups[0];
    const size_t total = staging_bytes(C);
    HIPCHK(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, sl.stream));
    LocateArgs x{};
    const ApplyArgs a = chunk_launch_args(C, d, 0, r.k, g.R, tabs + tab_off[2], g.tab_stride, x.r);
    x.r.vmask = reinterpret_cast<const uint32_t*>(tabs + tab_off[0]);
    x.nrows = reinterpret_cast<const uint32_t*>(tabs + tab_off[1]);
    x.gf = tabs + tab_off[3];
    x.loc = tabs + tab_off[4];
    x.counts = reinterpret_cast<uint64_t*>(d + locate_counts_off(C));
    x.loc_stride = static_cast<uint32_t>(r.t.stride);
    x.nbins = static_cast<uint32_t>(r.bins());
    HIPCHK(r.repair ? launch_correct(a, x, C.any_tail, sl.stream)
                    : launch_locate(a, x, C.any_tail, sl.stream, {}, r.t.max_errors));
    HIPCHK(hipMemcpyAsync(h + C.status_off, d + C.status_off, total - C.status_off, hipMemcpyDeviceToHost,
                          sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_launches.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_copies.fetch_add(2, std::memory_order_relaxed);
    return RS_OK;
  }

  // The flags and the counts; then, a correct run, the repaired rows while the chunk's device
  // mirror still stands.
  int collect(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>&) {
    const uint8_t* h = staging(sl);
    const int* st = reinterpret_cast<const int*>(h + C.status_off);
    const uint64_t* cn = reinterpret_cast<const uint64_t*>(h + locate_counts_off(C));
    const size_t k = static_cast<size_t>(r.k), n = static_cast<size_t>(r.k + r.m), nb = r.bins();
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const size_t id = static_cast<size_t>(r.ids[static_cast<size_t>(it.stripe)]);
      if (st[j]) flags[id] = 1;
      for (size_t q = 0; q < nb; ++q) counts[id * nb + q] += cn[j * nb + q];
      if (!r.repair) continue;
      const MixedPattern& pt = r.mt().patterns[pattern(C, j)];
      for (size_t row = 0; row < k + r.t.rows(pattern(C, j)); ++row) {
        const size_t shard = static_cast<size_t>(row < k ? pt.valid[row] : pt.rows[row - k]);
        if (cn[j * nb + shard] == 0) continue;
        HIPCHK(hipMemcpy(r.repair[id * n + shard] + it.off, base(sl) + C.items[j].in_off + C.items[j].pitch * row,
                         it.w, hipMemcpyDeviceToHost));
        r.ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
      }
    }
    return RS_OK;
  }
};

// The call's runnable stripes `ids` (each has more than k present shards, a nonzero size and
// its pointers) on one device and lane. sizes and present (0 / 1 flags, batch * (k + m)) are
// the whole call's; counts too, zeroed by the caller. max_errors 1 or 2 (2: pair tables and the
// pair kernel). repair (with max_errors 1): a correct run, the call's shards.
template <class ShardF>
int run_locate(rs_ctx* ctx, int k, int m, int max_errors, const std::vector<int>& ids, const size_t* sizes,
               const uint8_t* present, ShardF shard_of, uint64_t* counts, int* flags,
               uint8_t* const* repair = nullptr) {
  if (ids.empty()) return RS_OK;
  if (ctx->devs.empty()) return RS_E_HIP;
  ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  ctx->n_ragged_calls.fetch_add(1, std::memory_order_relaxed);
  Device* dev = ctx->devs[device_slot(ctx->rr.fetch_add(1), 0, ctx->devs.size())].get();
  // the runnable stripes' sizes and presence rows: what a run is keyed by
  const size_t n = static_cast<size_t>(k + m);
  std::vector<size_t> sz(ids.size());
  std::vector<uint8_t> pres(ids.size() * n);
  for (size_t j = 0; j < ids.size(); ++j) {
    sz[j] = sizes[ids[j]];
    std::memcpy(&pres[j * n], present + static_cast<size_t>(ids[j]) * n, n);
  }
  const size_t per = pattern_arena_bytes(k, kLocateRows) + locate_stride(k, max_errors);
  return with_lane(ctx, dev, [&](Lane& L) -> int {
    HIPCHK(hipSetDevice(dev->id));
    return for_each_run(ids, n, per, pres.data(), [&](size_t begin, size_t end) -> int {
      LocateRun r{ctx, k, m, {}, {}, {}, repair};
      r.ids.assign(ids.begin() + static_cast<ptrdiff_t>(begin), ids.begin() + static_cast<ptrdiff_t>(end));
      const std::vector<size_t> rsz(sz.begin() + static_cast<ptrdiff_t>(begin), sz.begin() + static_cast<ptrdiff_t>(end));
      const TableError te =
          build_locate_tables(k, m, static_cast<int>(end - begin), rsz.data(), &pres[begin * n], r.t, max_errors);
      if (te == TableError::kSingular) return RS_E_SINGULAR;
      if (te != TableError::kOk || r.mt().groups.size() != 1) return RS_E_ARG;
      r.sh = ragged_shape(k, r.mt().groups, rsz, [&](int s) {
        return std::make_pair(k + static_cast<int>(r.t.rows(r.mt().pat[static_cast<size_t>(s)])), 0);
      });
      RaggedWork w(r.sh, chunk_bytes());
      if (!w.cut(r.sh, chunk_bytes())) return RS_E_ARG;
      LocateJob<ShardF> job(r, L, w.items, shard_of, counts, flags);
      return run_chunk_pipeline(ctx, L, w.chunks, job);
    });
  });
}

}  // namespace
}  // namespace callfs
