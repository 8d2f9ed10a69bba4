// Update / EncodeIdx on host memory: rs_update, rs_encode_idx,
// rs_update_batch and rs_codec_overwrite are one route, the ragged pipeline of §7.5 on its
// staged transport. The stripes with a changed shard become items (ragged_chunks.hpp: whole
// stripes, or column parts of stripes too large for a chunk); a chunk stages its items' changed
// sources as input rows and their m parity rows as output rows, moves with one H2D (sources,
// parity and metadata), runs launch_update per launch group on the slot's device mirror and
// brings the parity rows back with one D2H. Included by rs_host.cpp only.
#pragma once

#include "host_common.hpp"
#include "ragged_chunks.hpp"
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

// The run's arenas and source counts in the lane's device buffer: [nsrc], then per launch
// group its arena; uploaded when the lane last held other tables (the ragged runs' keys start
// with a digit).
struct UpdateDevTables {
  size_t nsrc_off = 0;
  std::vector<size_t> arena_off;
};
int upload_update_tables(const UpdateRun& r, Lane& L, UpdateDevTables& dt) {
  Packer pk;
  dt.nsrc_off = pk.take(sizeof(uint32_t) * r.t.nsrc.size());
  for (const UpdateGroup& g : r.t.groups) dt.arena_off.push_back(pk.take(g.arena.size()));
  std::string key = "U" + std::to_string(r.k) + "," + std::to_string(r.m) + "," + std::to_string(r.t.cmax) + ":";
  for (const std::vector<int>& p : r.t.patterns) {
    for (int i : p) key.push_back(static_cast<char>(i));
    key.push_back('|');
    key.push_back(static_cast<char>(p.size()));  // (an index can be '|')
  }
  if (L.rag_tabs.p && L.rag_key == key) return RS_OK;
  L.rag_key.clear();
  if (const int rc = L.rag_tabs.ensure(pk.off)) return rc;
  std::vector<uint8_t> h(pk.off, 0);
  std::memcpy(h.data() + dt.nsrc_off, r.t.nsrc.data(), sizeof(uint32_t) * r.t.nsrc.size());
  for (size_t gi = 0; gi < r.t.groups.size(); ++gi)
    std::memcpy(h.data() + dt.arena_off[gi], r.t.groups[gi].arena.data(), r.t.groups[gi].arena.size());
  HIPCHK(hipMemcpy(L.rag_tabs.p, h.data(), h.size(), hipMemcpyHostToDevice));
  r.ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
  L.rag_key = std::move(key);
  return RS_OK;
}

// The chunk's metadata at h; the pointers name the rows at the same offsets from d.
void fill_update_meta(const UpdateRun& r, const ChunkLayout& C, const std::vector<RaggedItem>& items,
                      uint8_t* h, uint8_t* d) {
  const size_t stride = r.in_stride();
  auto* in = reinterpret_cast<const uint8_t**>(h + C.in_tab_off);
  auto* pat = reinterpret_cast<uint32_t*>(h + C.pat_off);
  auto* size = reinterpret_cast<uint64_t*>(h + C.size_off);
  std::vector<size_t> widths(C.count);
  for (size_t j = 0; j < C.count; ++j) {
    const RaggedItem& it = items[C.first + j];
    const ItemLayout& il = C.items[j];
    widths[j] = it.w;
    size[j] = it.w;
    pat[j] = r.t.pat[static_cast<size_t>(it.stripe)];
    const size_t rows = static_cast<size_t>(r.sh.nin[static_cast<size_t>(it.stripe)]);
    for (size_t q = 0; q < stride; ++q) in[j * stride + q] = q < rows ? d + il.in_off + il.pitch * q : nullptr;
  }
  for (size_t gi = 0; gi < r.t.groups.size(); ++gi) {
    const UpdateGroup& g = r.t.groups[gi];
    auto* out = reinterpret_cast<uint8_t**>(h + C.out_tab_off[gi]);
    for (size_t j = 0; j < C.count; ++j)
      for (int row = 0; row < g.R; ++row)
        out[j * static_cast<size_t>(g.R) + row] =
            d + C.items[j].out_off + C.items[j].pitch * static_cast<size_t>(g.row0 + row);
  }
  TileMap tm;
  (void)build_tile_map(static_cast<int>(C.count), widths.data(), nullptr, tm);
  std::memcpy(h + C.tile0_off, tm.tile0.data(), sizeof(uint32_t) * tm.tile0.size());
  std::memcpy(h + C.tile_stripe_off, tm.tile_stripe.data(), sizeof(uint32_t) * tm.tile_stripe.size());
}

// The chunk loop, in the style of run_ragged_chunks: chunks rotate through the lane's slots;
// the parity rows of the chunk a slot held before leave its staging before the next chunk's
// layout overwrites them. old_of / new_of / par_of take a stripe of the call and a shard or
// parity row index.
template <class OldF, class NewF, class ParF>
int run_update_chunks(const UpdateRun& r, Lane& L, const std::vector<RaggedItem>& items,
                      const std::vector<ChunkLayout>& chunks, OldF& old_of, NewF& new_of, ParF& par_of) {
  int rc;
  UpdateDevTables dt;
  if ((rc = upload_update_tables(r, L, dt))) return rc;
  size_t bytes = 0;
  for (const ChunkLayout& C : chunks) bytes = std::max(bytes, C.out_end);
  const size_t nchunks = chunks.size();
  const size_t nslots = std::min<size_t>(nchunks, static_cast<size_t>(pipeline_slots()));
  for (size_t si = 0; si < nslots; ++si) {
    Slot& sl = L.slot[si];
    if ((rc = sl.dev.ensure(bytes)) || (rc = sl.host.ensure(bytes))) return rc;
    sl.pending = false;
  }
  const uint8_t* tabs = static_cast<const uint8_t*>(L.rag_tabs.p);
  std::vector<CopyPool::Seg> segs;
  auto drain = [&](Slot& sl) -> int {
    if (!sl.pending) return RS_OK;
    HIPCHK(hipEventSynchronize(sl.done));
    const ChunkLayout& C = chunks[sl.rag_chunk];
    uint8_t* h = static_cast<uint8_t*>(sl.host.p);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      for (int row = 0; row < r.m; ++row)
        segs.push_back({par_of(id, row) + it.off,
                        h + C.items[j].out_off + C.items[j].pitch * static_cast<size_t>(row), it.w});
    }
    sl.pending = false;
    return RS_OK;
  };
  for (size_t c = 0; c < nchunks; ++c) {
    Slot& sl = L.slot[c % nslots];
    segs.clear();
    if ((rc = drain(sl))) return rc;
    if (!segs.empty()) r.ctx->pool.run(segs);
    segs.clear();
    const ChunkLayout& C = chunks[c];
    uint8_t* h = static_cast<uint8_t*>(sl.host.p);
    uint8_t* d = static_cast<uint8_t*>(sl.dev.p);
    fill_update_meta(r, C, items, h, d);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      const std::vector<int>& idx = r.t.patterns[r.t.pat[static_cast<size_t>(it.stripe)]];
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
    r.ctx->pool.run(segs);
    // one H2D of metadata, sources and parity; the launches; one D2H of the parity rows
    const size_t rows0 = C.items[0].out_off;
    HIPCHK(hipMemcpyAsync(d, h, C.out_end, hipMemcpyHostToDevice, sl.stream));
    for (size_t gi = 0; gi < r.t.groups.size(); ++gi) {
      const UpdateGroup& g = r.t.groups[gi];
      ApplyArgs a{};
      a.in_tab = reinterpret_cast<const uint8_t* const*>(d + C.in_tab_off);
      a.out_tab = reinterpret_cast<uint8_t* const*>(d + C.out_tab_off[gi]);
      a.ltabs = tabs + dt.arena_off[gi];
      a.K = r.t.cmax;
      a.R = g.R;
      a.batch = static_cast<int>(C.count);
      UpdateArgs x{};
      x.pat = reinterpret_cast<const uint32_t*>(d + C.pat_off);
      x.nsrc = reinterpret_cast<const uint32_t*>(tabs + dt.nsrc_off);
      x.size = reinterpret_cast<const uint64_t*>(d + C.size_off);
      x.tile0 = reinterpret_cast<const uint32_t*>(d + C.tile0_off);
      x.tile_stripe = reinterpret_cast<const uint32_t*>(d + C.tile_stripe_off);
      x.tab_stride = static_cast<uint32_t>(g.tab_stride);
      x.ntiles = C.ntiles;
      x.in_stride = static_cast<uint32_t>(r.in_stride());
      HIPCHK(launch_update(a, x, r.pair, C.any_tail, sl.stream));
    }
    HIPCHK(hipMemcpyAsync(h + rows0, d + rows0, C.out_end - rows0, hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_launches.fetch_add(r.t.groups.size(), std::memory_order_relaxed);
    r.ctx->n_copies.fetch_add(2, std::memory_order_relaxed);
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
  return with_lane(ctx, dev, [&](Lane& L) -> int {
    HIPCHK(hipSetDevice(dev->id));
    // segments whose distinct changed sets' tables stay within the arena budget (sized as if
    // every set were all k shards)
    const size_t max_patterns =
        std::max<size_t>(1, kRaggedArenaBudget / std::max<size_t>(1, pattern_arena_bytes(k, m)));
    size_t begin = 0;
    while (begin < ids.size()) {
      std::set<std::string> seen;
      size_t end = begin;
      for (; end < ids.size(); ++end) {
        std::string key(reinterpret_cast<const char*>(changed + static_cast<size_t>(ids[end]) * k),
                        static_cast<size_t>(k));
        for (char& ch : key) ch = ch ? 1 : 0;
        if (!seen.count(key) && seen.size() == max_patterns) break;
        seen.insert(std::move(key));
      }
      UpdateRun r{ctx, k, m, pair, {}, {}, {}};
      r.ids.assign(ids.begin() + static_cast<ptrdiff_t>(begin), ids.begin() + static_cast<ptrdiff_t>(end));
      const int count = static_cast<int>(r.ids.size());
      std::vector<size_t> sz(r.ids.size());
      std::vector<uint8_t> ch(r.ids.size() * static_cast<size_t>(k));
      for (size_t s = 0; s < r.ids.size(); ++s) {
        sz[s] = sizes[r.ids[s]];
        std::memcpy(&ch[s * k], changed + static_cast<size_t>(r.ids[s]) * k, static_cast<size_t>(k));
      }
      const TableError te = build_update_tables(k, m, count, sz.data(), ch.data(), r.t);
      if (te == TableError::kSingular) return RS_E_SINGULAR;
      if (te != TableError::kOk) return RS_E_ARG;
      r.sh.k = static_cast<int>(r.in_stride());
      for (const UpdateGroup& g : r.t.groups) r.sh.group_rows.push_back(g.R);
      for (int s = 0; s < count; ++s) {
        r.sh.size.push_back(sz[static_cast<size_t>(s)]);
        r.sh.nin.push_back(static_cast<int>(r.t.nsrc[r.t.pat[static_cast<size_t>(s)]]) * (pair ? 2 : 1));
        r.sh.nout.push_back(m);
      }
      const std::vector<RaggedItem> items = ragged_items(r.sh, chunk_bytes());
      const std::vector<ChunkLayout> chunks = ragged_chunks(r.sh, items, chunk_bytes());
      for (const ChunkLayout& C : chunks)
        if (C.ntiles > kRaggedMaxTiles) return RS_E_ARG;
      if (const int rc = run_update_chunks(r, L, items, chunks, old_of, new_of, par_of)) return rc;
      begin = end;
    }
    return RS_OK;
  });
}

}  // namespace
}  // namespace callfs
