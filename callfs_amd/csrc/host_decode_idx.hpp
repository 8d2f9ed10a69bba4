// DecodeIdx on host memory: rs_decode_idx and rs_decode_idx_batch are one
// route, a job of the chunk pipeline of §7.5 (host_chunks.hpp) on the staged transport's slots.
// The stripes with both a delivered and a wanted shard become items (ragged_chunks.hpp: whole
// stripes, or column parts of stripes too large for a chunk -- columns are independent); a chunk
// stages its items' delivered shards as input rows and their wanted shards as output rows, uploads
// them, runs launch_decode_idx per launch group on the slot's device mirror and brings
// the wanted rows back with one D2H. The upload is one H2D of the metadata and the inputs and, in
// merge mode alone, a second H2D of the wanted rows' current bytes: a store chunk does not upload
// them, and rs_host_counters' `copies` shows it (2 per store chunk, 3 per merge chunk).
// Included by rs_host.cpp only.
#pragma once

#include "decode_idx_tables.hpp"
#include "host_chunks.hpp"

namespace callfs {
namespace {

// One run: consecutive runnable stripes whose pattern tables fit kRaggedArenaBudget. Stripe s of
// the run is stripe ids[s] of the call.
struct DecodeIdxRun {
  rs_ctx* ctx;
  int k, m;
  bool store;
  DecodeIdxTables t;
  RaggedShape sh;  // k = source pointers per item (cmax); nin = delivered rows, nout = wanted rows
  std::vector<int> ids;
};

// The route's job. in_of / dst_of take a stripe of the call and a shard index.
template <class InF, class DstF>
struct DecodeIdxJob : StagedSlots {
  const DecodeIdxRun& r;
  Lane& L;
  const std::vector<RaggedItem>& items;
  InF& in_of;
  DstF& dst_of;
  std::vector<size_t> tab_off;  // in the lane's device buffer: [nsrc], then per launch group arena, [nrows]
  DecodeIdxJob(const DecodeIdxRun& run, Lane& lane, const std::vector<RaggedItem>& its, InF& i, DstF& d)
      : r(run), L(lane), items(its), in_of(i), dst_of(d) {}

  // (the ragged runs' keys start with a digit, the update runs' with 'U')
  int prepare_run() {
    std::vector<TablePiece> pieces{{r.t.nsrc.data(), sizeof(uint32_t) * r.t.nsrc.size()}};
    for (const DecodeIdxGroup& g : r.t.groups) {
      pieces.push_back({g.arena.data(), g.arena.size()});
      pieces.push_back({g.nrows.data(), sizeof(uint32_t) * g.nrows.size()});
    }
    std::string key = "D" + std::to_string(r.k) + "," + std::to_string(r.m) + "," + std::to_string(r.t.cmax) + "," +
                      std::to_string(r.t.rmax) + ":";
    for (const DecodeIdxPattern& p : r.t.patterns)
      for (const std::vector<int>* v : {&p.expect, &p.wanted, &p.delivered}) {
        for (int i : *v) key.push_back(static_cast<char>(i));
        key.push_back('|');
        key.push_back(static_cast<char>(v->size()));  // (an index can be '|')
      }
    return upload_lane_tables(r.ctx, L.rag_tabs, L.rag_key, std::move(key), pieces, tab_off);
  }
  size_t staging_bytes(const ChunkLayout& C) const { return C.out_end; }

  // The metadata (its pointers name the rows at the same offsets of the device mirror), the
  // delivered shards and, in merge mode, the wanted shards' current bytes.
  int stage(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const size_t stride = static_cast<size_t>(r.t.cmax);
    auto* in = reinterpret_cast<const uint8_t**>(h + C.in_tab_off);
    auto* pat = reinterpret_cast<uint32_t*>(h + C.pat_off);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      pat[j] = r.t.pat[static_cast<size_t>(it.stripe)];
      const DecodeIdxPattern& p = r.t.patterns[pat[j]];
      for (size_t q = 0; q < stride; ++q)
        in[j * stride + q] = q < p.delivered.size() ? d + il.in_off + il.pitch * q : nullptr;
      for (size_t q = 0; q < p.delivered.size(); ++q)
        segs.push_back({h + il.in_off + il.pitch * q, in_of(id, p.delivered[q]) + it.off, it.w});
      if (!r.store)
        for (size_t q = 0; q < p.wanted.size(); ++q)
          segs.push_back({h + il.out_off + il.pitch * q, dst_of(id, p.wanted[q]) + it.off, it.w});
    }
    for (size_t gi = 0; gi < r.t.groups.size(); ++gi) {
      const DecodeIdxGroup& g = r.t.groups[gi];
      auto* out = reinterpret_cast<uint8_t**>(h + C.out_tab_off[gi]);
      for (size_t j = 0; j < C.count; ++j)
        for (int row = 0; row < g.R; ++row)
          out[j * static_cast<size_t>(g.R) + row] =
              row < static_cast<int>(g.nrows[pat[j]])
                  ? d + C.items[j].out_off + C.items[j].pitch * static_cast<size_t>(g.row0 + row)
                  : nullptr;
    }
    fill_chunk_tile_map(C, items, h);
    return RS_OK;
  }

  // The H2D of metadata and inputs; merge: the H2D of the wanted rows; the launches; one D2H
  // from the first wanted row.
  int send(Slot& sl, const ChunkLayout& C) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const uint8_t* tabs = static_cast<const uint8_t*>(L.rag_tabs.p);
    const size_t rows0 = C.items[0].out_off;
    HIPCHK(hipMemcpyAsync(d, h, C.in_end, hipMemcpyHostToDevice, sl.stream));
    if (!r.store)
      HIPCHK(hipMemcpyAsync(d + rows0, h + rows0, C.out_end - rows0, hipMemcpyHostToDevice, sl.stream));
    for (size_t gi = 0; gi < r.t.groups.size(); ++gi) {
      const DecodeIdxGroup& g = r.t.groups[gi];
      MergeArgs x{};
      const ApplyArgs a =
          chunk_launch_args(C, d, gi, r.t.cmax, g.R, tabs + tab_off[1 + 2 * gi], g.tab_stride, x.u);
      x.u.nsrc = reinterpret_cast<const uint32_t*>(tabs + tab_off[0]);
      x.u.in_stride = static_cast<uint32_t>(r.t.cmax);
      x.nrows = reinterpret_cast<const uint32_t*>(tabs + tab_off[2 + 2 * gi]);
      HIPCHK(launch_decode_idx(a, x, r.store, C.any_tail, sl.stream));
    }
    HIPCHK(hipMemcpyAsync(h + rows0, d + rows0, C.out_end - rows0, hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_launches.fetch_add(r.t.groups.size(), std::memory_order_relaxed);
    r.ctx->n_copies.fetch_add(r.store ? 2 : 3, std::memory_order_relaxed);
    return RS_OK;
  }

  // The wanted rows, back into the caller's shards.
  int collect(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      const DecodeIdxPattern& p = r.t.patterns[r.t.pat[static_cast<size_t>(it.stripe)]];
      for (size_t q = 0; q < p.wanted.size(); ++q)
        segs.push_back({dst_of(id, p.wanted[q]) + it.off, h + C.items[j].out_off + C.items[j].pitch * q, it.w});
    }
    return RS_OK;
  }
};

// The call's runnable stripes `ids` (each has a delivered and a wanted shard, a nonzero size and
// k expected shards) on one device and lane. flags: batch * (k + m) bytes of the whole call,
// bit 0 expected, bit 1 delivered, bit 2 wanted.
template <class InF, class DstF>
int run_decode_idx(rs_ctx* ctx, int k, int m, bool store, const std::vector<int>& ids, const size_t* sizes,
                   const uint8_t* flags, InF in_of, DstF dst_of) {
  if (ids.empty()) return RS_OK;
  if (ctx->devs.empty()) return RS_E_HIP;
  ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  ctx->n_ragged_calls.fetch_add(1, std::memory_order_relaxed);
  Device* dev = ctx->devs[device_slot(ctx->rr.fetch_add(1), 0, ctx->devs.size())].get();
  const size_t n = static_cast<size_t>(k + m);
  std::vector<size_t> sz(ids.size());
  std::vector<uint8_t> fl(ids.size() * n);
  for (size_t j = 0; j < ids.size(); ++j) {
    sz[j] = sizes[ids[j]];
    std::memcpy(&fl[j * n], flags + static_cast<size_t>(ids[j]) * n, n);
  }
  return with_lane(ctx, dev, [&](Lane& L) -> int {
    HIPCHK(hipSetDevice(dev->id));
    // runs whose distinct patterns' tables stay within the arena budget (sized as if every
    // pattern delivered all k shards into m rows)
    return for_each_run(ids, n, pattern_arena_bytes(k, m), fl.data(), [&](size_t begin, size_t end) -> int {
      DecodeIdxRun r{ctx, k, m, store, {}, {}, {}};
      r.ids.assign(ids.begin() + static_cast<ptrdiff_t>(begin), ids.begin() + static_cast<ptrdiff_t>(end));
      const std::vector<size_t> rsz(sz.begin() + static_cast<ptrdiff_t>(begin), sz.begin() + static_cast<ptrdiff_t>(end));
      const size_t cells = (end - begin) * n;
      std::vector<uint8_t> ex(cells), hin(cells), hdst(cells);
      for (size_t i = 0; i < cells; ++i) {
        const uint8_t f = fl[begin * n + i];
        ex[i] = f & 1u;
        hin[i] = (f >> 1) & 1u;
        hdst[i] = (f >> 2) & 1u;
      }
      const DecodeIdxError te = build_decode_idx_tables(k, m, static_cast<int>(end - begin), rsz.data(), ex.data(),
                                                        hin.data(), hdst.data(), r.t);
      if (te == DecodeIdxError::kSingular) return RS_E_SINGULAR;
      if (te != DecodeIdxError::kOk) return RS_E_ARG;
      r.sh = ragged_shape(r.t.cmax, r.t.groups, rsz, [&](int s) {
        const uint32_t p = r.t.pat[static_cast<size_t>(s)];
        return std::make_pair(static_cast<int>(r.t.nsrc[p]), static_cast<int>(r.t.nrows[p]));
      });
      RaggedWork w(r.sh, chunk_bytes());
      if (!w.cut(r.sh, chunk_bytes())) return RS_E_ARG;
      DecodeIdxJob<InF, DstF> job(r, L, w.items, in_of, dst_of);
      return run_chunk_pipeline(ctx, L, w.chunks, job);
    });
  });
}

}  // namespace
}  // namespace callfs
