// DecodeIdx on host memory: rs_decode_idx and rs_decode_idx_batch are one
// route, a job of the chunk pipeline of §7.5 (host_chunks.hpp) on the staged transport's slots.
// The stripes with both a delivered and a wanted shard become items (ragged_chunks.hpp: whole
// stripes, or column parts of stripes too large for a chunk -- columns are independent); a chunk
// stages its items' delivered shards as input rows and their wanted shards as output rows, uploads
// them, runs launch_decode_idx per launch group on the slot's device mirror and brings
// the wanted rows back with one D2H. The upload is one H2D of the metadata and the inputs and, in
// merge mode alone, a second H2D of the wanted rows' current bytes: a store chunk does not upload
// them, and rs_host_counters' `copies` shows it (2 per store chunk, 3 per merge chunk).
// DecodeCheck on host memory (§5.15): rs_decode_check and rs_decode_check_batch are the same job
// over decode_check_tables.hpp. A compared shard's accumulator is one more output row: staged,
// uploaded in merge mode and, unless the call is final, downloaded like a wanted row. A final
// chunk also uploads its items' zeroed status words behind the inputs (the same H2D), runs
// launch_decode_check, brings the status words back in the D2H of the rows (the status words
// alone when the run has no wanted row) and copies no check row back; a flagged item flags its
// stripe, so a stripe cut into column parts ORs its parts' flags. `copies` is as for DecodeIdx,
// final or not: 2 per store chunk, 3 per merge chunk.
// Included by rs_host.cpp only.
#pragma once

#include <type_traits>

#include "decode_check_tables.hpp"
#include "decode_idx_tables.hpp"
#include "host_chunks.hpp"

namespace callfs {
namespace {

// One run: consecutive runnable stripes whose pattern tables fit kRaggedArenaBudget. Stripe s of
// the run is stripe ids[s] of the call.
// T: DecodeIdxTables, or DecodeCheckTables (then `final` may be set).
template <class T>
struct DecodeIdxRun {
  rs_ctx* ctx;
  int k, m;
  bool store, final;
  T t;
  RaggedShape sh;  // k = source pointers per item (cmax, at least 1); nin = delivered rows, nout = rows
  std::vector<int> ids;
  int stride() const { return std::max(1, t.cmax); }
};

inline const std::vector<int>& host_rows(const DecodeIdxPattern& p) { return p.wanted; }
inline const std::vector<int>& host_rows(const DecodeCheckPattern& p) { return p.rows; }
inline bool host_check_row(const DecodeIdxPattern&, size_t) { return false; }
inline bool host_check_row(const DecodeCheckPattern& p, size_t q) { return p.check[q] != 0; }
inline const std::vector<uint32_t>* host_cmask(const DecodeIdxGroup&) { return nullptr; }
inline const std::vector<uint32_t>* host_cmask(const DecodeCheckGroup& g) { return &g.cmask; }

// The route's job. in_of / dst_of take a stripe of the call and a shard index; dst_of gives a
// row's buffer, a wanted shard or a compared shard's accumulator. flags (a final run's): per
// stripe of the call, set when an item of it was flagged.
template <class T, class InF, class DstF>
struct DecodeIdxJob : StagedSlots {
  const DecodeIdxRun<T>& r;
  Lane& L;
  const std::vector<RaggedItem>& items;
  InF& in_of;
  DstF& dst_of;
  int* flags;
  // in the lane's device buffer: [nsrc], then per launch group arena, [nrows], [cmask]
  std::vector<size_t> tab_off;
  bool any_wanted = false;  // some pattern of the run has a row that is no check row
  DecodeIdxJob(const DecodeIdxRun<T>& run, Lane& lane, const std::vector<RaggedItem>& its, InF& i, DstF& d, int* fl)
      : r(run), L(lane), items(its), in_of(i), dst_of(d), flags(fl) {
    for (const auto& p : r.t.patterns)
      for (size_t q = 0; q < host_rows(p).size(); ++q) any_wanted |= !host_check_row(p, q);
  }

  // (the ragged runs' keys start with a digit, the update runs' with 'U')
  int prepare_run() {
    std::vector<TablePiece> pieces{{r.t.nsrc.data(), sizeof(uint32_t) * r.t.nsrc.size()}};
    constexpr bool check = std::is_same<T, DecodeCheckTables>::value;
    for (const auto& g : r.t.groups) {
      pieces.push_back({g.arena.data(), g.arena.size()});
      pieces.push_back({g.nrows.data(), sizeof(uint32_t) * g.nrows.size()});
      // (a decode-idx run keeps an empty third piece: one layout for both)
      const std::vector<uint32_t>* cm = host_cmask(g);
      pieces.push_back({cm ? cm->data() : nullptr, cm ? sizeof(uint32_t) * cm->size() : 0});
    }
    std::string key = (check ? "K" : "D") + std::to_string(r.k) + "," + std::to_string(r.m) + "," +
                      std::to_string(r.t.cmax) + "," + std::to_string(r.t.rmax) + ":";
    for (const auto& p : r.t.patterns) {
      for (const std::vector<int>* v : {&p.expect, &host_rows(p), &p.delivered}) {
        for (int i : *v) key.push_back(static_cast<char>(i));
        key.push_back('|');
        key.push_back(static_cast<char>(v->size()));  // (an index can be '|')
      }
      for (size_t q = 0; check && q < host_rows(p).size(); ++q) key.push_back(host_check_row(p, q) ? 'c' : 'w');
    }
    return upload_lane_tables(r.ctx, L.rag_tabs, L.rag_key, std::move(key), pieces, tab_off);
  }
  size_t staging_bytes(const ChunkLayout& C) const { return C.out_end; }

  // The metadata (its pointers name the rows at the same offsets of the device mirror), the
  // delivered shards and, in merge mode, the rows' current bytes; the zeroed status words.
  int stage(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const size_t stride = static_cast<size_t>(r.stride());
    auto* in = reinterpret_cast<const uint8_t**>(h + C.in_tab_off);
    auto* pat = reinterpret_cast<uint32_t*>(h + C.pat_off);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      pat[j] = r.t.pat[static_cast<size_t>(it.stripe)];
      const auto& p = r.t.patterns[pat[j]];
      for (size_t q = 0; q < stride; ++q)
        in[j * stride + q] = q < p.delivered.size() ? d + il.in_off + il.pitch * q : nullptr;
      for (size_t q = 0; q < p.delivered.size(); ++q)
        segs.push_back({h + il.in_off + il.pitch * q, in_of(id, p.delivered[q]) + it.off, it.w});
      if (!r.store)
        for (size_t q = 0; q < host_rows(p).size(); ++q)
          segs.push_back({h + il.out_off + il.pitch * q, dst_of(id, host_rows(p)[q]) + it.off, it.w});
    }
    for (size_t gi = 0; gi < r.t.groups.size(); ++gi) {
      const auto& g = r.t.groups[gi];
      auto* out = reinterpret_cast<uint8_t**>(h + C.out_tab_off[gi]);
      for (size_t j = 0; j < C.count; ++j)
        for (int row = 0; row < g.R; ++row)
          out[j * static_cast<size_t>(g.R) + row] =
              row < static_cast<int>(g.nrows[pat[j]])
                  ? d + C.items[j].out_off + C.items[j].pitch * static_cast<size_t>(g.row0 + row)
                  : nullptr;
    }
    fill_chunk_tile_map(C, items, h);
    std::memset(h + C.status_off, 0, sizeof(int) * C.count);
    return RS_OK;
  }

  // The H2D of metadata and inputs (final: through the status words); merge: the H2D of the
  // rows; the launches; one D2H from the first row (final: from the status words, and of them
  // alone when the run has no wanted row).
  int send(Slot& sl, const ChunkLayout& C) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const uint8_t* tabs = static_cast<const uint8_t*>(L.rag_tabs.p);
    const size_t rows0 = C.items[0].out_off;
    HIPCHK(hipMemcpyAsync(d, h, r.final ? C.status_off + sizeof(int) * C.count : C.in_end, hipMemcpyHostToDevice,
                          sl.stream));
    if (!r.store)
      HIPCHK(hipMemcpyAsync(d + rows0, h + rows0, C.out_end - rows0, hipMemcpyHostToDevice, sl.stream));
    for (size_t gi = 0; gi < r.t.groups.size(); ++gi) {
      const auto& g = r.t.groups[gi];
      MergeArgs x{};
      const ApplyArgs a =
          chunk_launch_args(C, d, gi, r.stride(), g.R, tabs + tab_off[1 + 3 * gi], g.tab_stride, x.u);
      x.u.nsrc = reinterpret_cast<const uint32_t*>(tabs + tab_off[0]);
      x.u.in_stride = static_cast<uint32_t>(r.stride());
      x.nrows = reinterpret_cast<const uint32_t*>(tabs + tab_off[2 + 3 * gi]);
      if (r.final)
        HIPCHK(launch_decode_check(a, CheckArgs{x, reinterpret_cast<const uint32_t*>(tabs + tab_off[3 + 3 * gi])},
                                   r.store, C.any_tail, sl.stream));
      else
        HIPCHK(launch_decode_idx(a, x, r.store, C.any_tail, sl.stream));
    }
    if (!r.final)
      HIPCHK(hipMemcpyAsync(h + rows0, d + rows0, C.out_end - rows0, hipMemcpyDeviceToHost, sl.stream));
    else
      HIPCHK(hipMemcpyAsync(h + C.status_off, d + C.status_off,
                            (any_wanted ? C.out_end : C.status_off + sizeof(int) * C.count) - C.status_off,
                            hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_launches.fetch_add(r.t.groups.size(), std::memory_order_relaxed);
    r.ctx->n_copies.fetch_add(r.store ? 2 : 3, std::memory_order_relaxed);
    return RS_OK;
  }

  // The rows, back into the caller's buffers; of a final chunk the wanted rows alone, and its
  // items' flags.
  int collect(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    const int* st = reinterpret_cast<const int*>(h + C.status_off);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      const auto& p = r.t.patterns[r.t.pat[static_cast<size_t>(it.stripe)]];
      if (r.final && st[j]) flags[id] = 1;
      for (size_t q = 0; q < host_rows(p).size(); ++q)
        if (!(r.final && host_check_row(p, q)))
          segs.push_back({dst_of(id, host_rows(p)[q]) + it.off, h + C.items[j].out_off + C.items[j].pitch * q, it.w});
    }
    return RS_OK;
  }
};

// The call's runnable stripes `ids` (each is in the launch, with a nonzero size and k expected
// shards) on one device and lane. flags: batch * (k + m) bytes of the whole call, bit 0 expected,
// bit 1 delivered, bit 2 wanted, bit 3 compared (T = DecodeCheckTables only). corrupt (a final
// call's): per stripe of the call, set when the stripe was flagged.
template <class T, class InF, class DstF>
int run_decode_idx(rs_ctx* ctx, int k, int m, bool store, bool final, const std::vector<int>& ids,
                   const size_t* sizes, const uint8_t* flags, InF in_of, DstF dst_of, int* corrupt = nullptr) {
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
      DecodeIdxRun<T> r{ctx, k, m, store, final, {}, {}, {}};
      r.ids.assign(ids.begin() + static_cast<ptrdiff_t>(begin), ids.begin() + static_cast<ptrdiff_t>(end));
      const std::vector<size_t> rsz(sz.begin() + static_cast<ptrdiff_t>(begin), sz.begin() + static_cast<ptrdiff_t>(end));
      const size_t cells = (end - begin) * n;
      std::vector<uint8_t> ex(cells), hin(cells), hdst(cells), hchk(cells);
      for (size_t i = 0; i < cells; ++i) {
        const uint8_t f = fl[begin * n + i];
        ex[i] = f & 1u;
        hin[i] = (f >> 1) & 1u;
        hdst[i] = (f >> 2) & 1u;
        hchk[i] = (f >> 3) & 1u;
      }
      DecodeIdxError te;
      if constexpr (std::is_same<T, DecodeCheckTables>::value)
        te = build_decode_check_tables(k, m, static_cast<int>(end - begin), rsz.data(), ex.data(), hin.data(),
                                       hdst.data(), hchk.data(), final, r.t);
      else
        te = build_decode_idx_tables(k, m, static_cast<int>(end - begin), rsz.data(), ex.data(), hin.data(),
                                     hdst.data(), r.t);
      if (te == DecodeIdxError::kSingular) return RS_E_SINGULAR;
      if (te != DecodeIdxError::kOk) return RS_E_ARG;
      r.sh = ragged_shape(r.stride(), r.t.groups, rsz, [&](int s) {
        const uint32_t p = r.t.pat[static_cast<size_t>(s)];
        return std::make_pair(static_cast<int>(r.t.nsrc[p]), static_cast<int>(r.t.nrows[p]));
      });
      RaggedWork w(r.sh, chunk_bytes());
      if (!w.cut(r.sh, chunk_bytes())) return RS_E_ARG;
      DecodeIdxJob<T, InF, DstF> job(r, L, w.items, in_of, dst_of, corrupt);
      return run_chunk_pipeline(ctx, L, w.chunks, job);
    });
  });
}

}  // namespace
}  // namespace callfs
