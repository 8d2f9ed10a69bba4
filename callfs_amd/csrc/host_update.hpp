// Update / EncodeIdx on host memory: rs_update, rs_encode_idx,
// rs_update_batch and rs_codec_overwrite are one route, a job of the chunk pipeline of §7.5
// (host_chunks.hpp) on the staged transport's slots. The stripes with a changed shard become
// items (ragged_chunks.hpp: whole stripes, or column parts of stripes too large for a chunk); a
// chunk stages its items' changed sources as input rows and their m parity rows as output rows,
// moves with one H2D (sources, parity and metadata), runs launch_update per launch group on the
// slot's device mirror and brings the parity rows back with one D2H. Included by rs_host.cpp only.
#pragma once

#include "host_chunks.hpp"
#include "update_tables.hpp"

namespace callfs {
namespace {

// One run: consecutive changed stripes whose pattern tables fit kRaggedArenaBudget. Stripe s of
// the run is stripe ids[s] of the call.
struct UpdateRun {
  rs_ctx* ctx;
  int k, m;
  bool pair;
  UpdateTables t;
  RaggedShape sh;  // k = source pointers per item; nin = the stripe's source rows, nout = m
  std::vector<int> ids;
  size_t in_stride() const { return static_cast<size_t>(t.cmax) * (pair ? 2 : 1); }
};

// The route's job. old_of / new_of / par_of take a stripe of the call and a shard or parity row
// index.
template <class OldF, class NewF, class ParF>
struct UpdateJob : StagedSlots {
  const UpdateRun& r;
  Lane& L;
  const std::vector<RaggedItem>& items;
  OldF& old_of;
  NewF& new_of;
  ParF& par_of;
  std::vector<size_t> tab_off;  // in the lane's device buffer: [nsrc], then per launch group its arena
  UpdateJob(const UpdateRun& run, Lane& lane, const std::vector<RaggedItem>& its, OldF& o, NewF& n, ParF& p)
      : r(run), L(lane), items(its), old_of(o), new_of(n), par_of(p) {}

  // (the ragged runs' keys start with a digit)
  int prepare_run() {
    std::vector<TablePiece> pieces{{r.t.nsrc.data(), sizeof(uint32_t) * r.t.nsrc.size()}};
    for (const UpdateGroup& g : r.t.groups) pieces.push_back({g.arena.data(), g.arena.size()});
    std::string key = "U" + std::to_string(r.k) + "," + std::to_string(r.m) + "," + std::to_string(r.t.cmax) + ":";
    for (const std::vector<int>& p : r.t.patterns) {
      for (int i : p) key.push_back(static_cast<char>(i));
      key.push_back('|');
      key.push_back(static_cast<char>(p.size()));  // (an index can be '|')
    }
    return upload_lane_tables(r.ctx, L.rag_tabs, L.rag_key, std::move(key), pieces, tab_off);
  }
  size_t staging_bytes(const ChunkLayout& C) const { return C.out_end; }

  // The metadata (its pointers name the rows at the same offsets of the device mirror), the
  // changed sources (old, new) and the parity rows.
  int stage(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const size_t stride = r.in_stride();
    auto* in = reinterpret_cast<const uint8_t**>(h + C.in_tab_off);
    auto* pat = reinterpret_cast<uint32_t*>(h + C.pat_off);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      pat[j] = r.t.pat[static_cast<size_t>(it.stripe)];
      const size_t rows = static_cast<size_t>(r.sh.nin[static_cast<size_t>(it.stripe)]);
      for (size_t q = 0; q < stride; ++q) in[j * stride + q] = q < rows ? d + il.in_off + il.pitch * q : nullptr;
      const std::vector<int>& idx = r.t.patterns[pat[j]];
      for (size_t q = 0; q < idx.size(); ++q) {
        if (r.pair) {
          segs.push_back({h + il.in_off + il.pitch * (2 * q), old_of(id, idx[q]) + it.off, it.w});
          segs.push_back({h + il.in_off + il.pitch * (2 * q + 1), new_of(id, idx[q]) + it.off, it.w});
        } else {
          segs.push_back({h + il.in_off + il.pitch * q, new_of(id, idx[q]) + it.off, it.w});
        }
      }
      for (int row = 0; row < r.m; ++row)
        segs.push_back({h + il.out_off + il.pitch * static_cast<size_t>(row), par_of(id, row) + it.off, it.w});
    }
    for (size_t gi = 0; gi < r.t.groups.size(); ++gi) {
      const UpdateGroup& g = r.t.groups[gi];
      auto* out = reinterpret_cast<uint8_t**>(h + C.out_tab_off[gi]);
      for (size_t j = 0; j < C.count; ++j)
        for (int row = 0; row < g.R; ++row)
          out[j * static_cast<size_t>(g.R) + row] =
              d + C.items[j].out_off + C.items[j].pitch * static_cast<size_t>(g.row0 + row);
    }
    fill_chunk_tile_map(C, items, h);
    return RS_OK;
  }

  // One H2D of metadata, sources and parity; the launches; one D2H from the first parity row.
  int send(Slot& sl, const ChunkLayout& C) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const uint8_t* tabs = static_cast<const uint8_t*>(L.rag_tabs.p);
    const size_t rows0 = C.items[0].out_off;
    HIPCHK(hipMemcpyAsync(d, h, C.out_end, hipMemcpyHostToDevice, sl.stream));
    for (size_t gi = 0; gi < r.t.groups.size(); ++gi) {
      const UpdateGroup& g = r.t.groups[gi];
      UpdateArgs x{};
      const ApplyArgs a = chunk_launch_args(C, d, gi, r.t.cmax, g.R, tabs + tab_off[1 + gi], g.tab_stride, x);
      x.nsrc = reinterpret_cast<const uint32_t*>(tabs + tab_off[0]);
      x.in_stride = static_cast<uint32_t>(r.in_stride());
      HIPCHK(launch_update(a, x, r.pair, C.any_tail, sl.stream));
    }
    HIPCHK(hipMemcpyAsync(h + rows0, d + rows0, C.out_end - rows0, hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_launches.fetch_add(r.t.groups.size(), std::memory_order_relaxed);
    r.ctx->n_copies.fetch_add(2, std::memory_order_relaxed);
    return RS_OK;
  }

  // The parity rows, back where they were staged from.
  int collect(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      for (int row = 0; row < r.m; ++row)
        segs.push_back({par_of(id, row) + it.off,
                        h + C.items[j].out_off + C.items[j].pitch * static_cast<size_t>(row), it.w});
    }
    return RS_OK;
  }
};

// The call's runnable stripes `ids` (each has a changed shard, a nonzero size and its pointers)
// on one device and lane. changed: batch * k flags of the whole call.
template <class OldF, class NewF, class ParF>
int run_update(rs_ctx* ctx, int k, int m, bool pair, const std::vector<int>& ids, const size_t* sizes,
               const uint8_t* changed, OldF old_of, NewF new_of, ParF par_of) {
  if (ids.empty()) return RS_OK;
  if (ctx->devs.empty()) return RS_E_HIP;
  ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  ctx->n_ragged_calls.fetch_add(1, std::memory_order_relaxed);
  Device* dev = ctx->devs[device_slot(ctx->rr.fetch_add(1), 0, ctx->devs.size())].get();
  // the runnable stripes' sizes and changed sets, as 0 / 1 rows: what a run is keyed by
  const size_t K = static_cast<size_t>(k);
  std::vector<size_t> sz(ids.size());
  std::vector<uint8_t> ch(ids.size() * K);
  for (size_t j = 0; j < ids.size(); ++j) {
    sz[j] = sizes[ids[j]];
    for (size_t i = 0; i < K; ++i) ch[j * K + i] = changed[static_cast<size_t>(ids[j]) * K + i] != 0;
  }
  return with_lane(ctx, dev, [&](Lane& L) -> int {
    HIPCHK(hipSetDevice(dev->id));
    // runs whose distinct changed sets' tables stay within the arena budget (sized as if every
    // set were all k shards)
    return for_each_run(ids, K, pattern_arena_bytes(k, m), ch.data(), [&](size_t begin, size_t end) -> int {
      UpdateRun r{ctx, k, m, pair, {}, {}, {}};
      r.ids.assign(ids.begin() + static_cast<ptrdiff_t>(begin), ids.begin() + static_cast<ptrdiff_t>(end));
      const std::vector<size_t> rsz(sz.begin() + static_cast<ptrdiff_t>(begin), sz.begin() + static_cast<ptrdiff_t>(end));
      const TableError te = build_update_tables(k, m, static_cast<int>(end - begin), rsz.data(), &ch[begin * K], r.t);
      if (te == TableError::kSingular) return RS_E_SINGULAR;
      if (te != TableError::kOk) return RS_E_ARG;
      r.sh = ragged_shape(static_cast<int>(r.in_stride()), r.t.groups, rsz, [&](int s) {
        return std::make_pair(static_cast<int>(r.t.nsrc[r.t.pat[static_cast<size_t>(s)]]) * (pair ? 2 : 1), m);
      });
      RaggedWork w(r.sh, chunk_bytes());
      if (!w.cut(r.sh, chunk_bytes())) return RS_E_ARG;
      UpdateJob<OldF, NewF, ParF> job(r, L, w.items, old_of, new_of, par_of);
      return run_chunk_pipeline(ctx, L, w.chunks, job);
    });
  });
}

}  // namespace
}  // namespace callfs
