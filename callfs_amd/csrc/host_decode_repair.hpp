// DecodeRepair on host memory: rs_decode_repair and rs_decode_repair_batch are
// a run of host_decode_idx.hpp's job on the staged transport, over decode_repair_tables.hpp. A
// chunk is a final decode-check chunk: the items' delivered shards as input rows, their wanted
// shards and their check accumulators as output rows (uploaded in merge mode alone), the zeroed
// status words behind the inputs. Behind the chunk's layout, as the locate route's counts, lie
// the fix pointer table (count * (k + 16) pointers, uploaded), the counts (count * (k + m + 1)
// words) and the fix rows, k + r' per item at the item's pitch, in the chunk's device mirror
// alone: counts and fix rows are zeroed on the device with one memset, and no fix row goes up.
// launch_decode_repair runs on the mirror; the status words and the wanted rows come back in one
// D2H, the counts in a second; then only the (item, shard) fix rows with a nonzero count whose
// fix buffer the caller gave are copied D2H, one copy each, while the mirror still stands, and
// XORed into the caller's buffer. A stripe cut into column parts adds its parts' counts and ORs
// their flags. `copies`: 4 per store chunk (metadata and inputs, fix table, rows back, counts
// back), 5 per merge chunk, plus one per fix row that came back. The fix rows are not part of
// what the chunk budget counts. Included by rs_host.cpp only.
#pragma once

#include "decode_repair_tables.hpp"
#include "host_decode_idx.hpp"

namespace callfs {
namespace {

struct DecodeRepairRun {
  rs_ctx* ctx;
  int k, m;
  bool store;
  DecodeRepairTables t;
  RaggedShape sh;  // k = source pointers per item (cmax, at least 1); nin = delivered rows, nout = rows
  std::vector<int> ids;
  int stride() const { return std::max(1, t.c.cmax); }
  size_t bins() const { return static_cast<size_t>(k + m) + 1; }
};

// Where a chunk's repair pieces lie behind its layout.
struct RepairOffsets {
  size_t fixtab = 0, counts = 0, rows = 0, total = 0;
  std::vector<size_t> item;  // [count] first fix row of item j; row q at item[j] + pitch * q
};

// in_of / dst_of as for DecodeIdxJob; fix_of gives the caller's fix buffer of a stripe's shard,
// or null. counts (the call's, batch * (k + m + 1)) are added into; flags[b] is set where an item
// of stripe b had a mismatching column.
template <class InF, class DstF, class FixF>
struct DecodeRepairJob : StagedSlots {
  const DecodeRepairRun& r;
  Lane& L;
  const std::vector<RaggedItem>& items;
  InF& in_of;
  DstF& dst_of;
  FixF& fix_of;
  uint64_t* counts;
  int* flags;
  std::vector<size_t> tab_off;  // in the lane's device buffer: [nsrc][arena][nrows][cmask][gf][loc]
  bool any_wanted = false;
  std::vector<uint8_t> row;  // one fix row on its way back
  DecodeRepairJob(const DecodeRepairRun& run, Lane& lane, const std::vector<RaggedItem>& its, InF& i, DstF& d, FixF& f,
                  uint64_t* cn, int* fl)
      : r(run), L(lane), items(its), in_of(i), dst_of(d), fix_of(f), counts(cn), flags(fl) {
    for (size_t p = 0; p < r.t.c.patterns.size(); ++p) any_wanted |= r.t.nchk[p] < r.t.c.patterns[p].rows.size();
  }

  uint32_t pattern(const ChunkLayout& C, size_t j) const {
    return r.t.c.pat[static_cast<size_t>(items[C.first + j].stripe)];
  }
  RepairOffsets offsets(const ChunkLayout& C) const {
    RepairOffsets o;
    o.fixtab = round_up(C.out_end, 256);
    o.counts = o.fixtab + sizeof(void*) * C.count * fix_slots(r.k);
    o.rows = round_up(o.counts + sizeof(uint64_t) * C.count * r.bins(), 256);
    size_t at = o.rows;
    for (size_t j = 0; j < C.count; ++j) {
      o.item.push_back(at);
      at += C.items[j].pitch * (static_cast<size_t>(r.k) + r.t.nchk[pattern(C, j)]);
    }
    o.total = at;
    return o;
  }

  // ("R": decode-repair runs' tables)
  int prepare_run() {
    const DecodeCheckGroup& g = r.t.c.groups[0];
    const std::vector<TablePiece> pieces{{r.t.c.nsrc.data(), sizeof(uint32_t) * r.t.c.nsrc.size()},
                                         {g.arena.data(), g.arena.size()},
                                         {g.nrows.data(), sizeof(uint32_t) * g.nrows.size()},
                                         {g.cmask.data(), sizeof(uint32_t) * g.cmask.size()},
                                         {r.t.gf.data(), r.t.gf.size()},
                                         {r.t.loc.data(), r.t.loc.size()}};
    std::string key = "R" + std::to_string(r.k) + "," + std::to_string(r.m) + "," + std::to_string(r.t.c.cmax) + "," +
                      std::to_string(r.t.c.rmax) + ":";
    for (size_t p = 0; p < r.t.c.patterns.size(); ++p) {
      const DecodeCheckPattern& pt = r.t.c.patterns[p];
      for (const std::vector<int>* v : {&pt.expect, &pt.rows, &pt.delivered}) {
        for (int i : *v) key.push_back(static_cast<char>(i));
        key.push_back('|');
        key.push_back(static_cast<char>(v->size()));  // (an index can be '|')
      }
      key.push_back(static_cast<char>(r.t.nchk[p]));
    }
    return upload_lane_tables(r.ctx, L.rag_tabs, L.rag_key, std::move(key), pieces, tab_off);
  }
  size_t staging_bytes(const ChunkLayout& C) const { return offsets(C).total; }

  // DecodeIdxJob's staging of a final chunk, and the fix pointer table: position q of item j
  // names the item's fix row q in the mirror where the caller gave that shard a fix buffer.
  int stage(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const RepairOffsets o = offsets(C);
    const size_t stride = static_cast<size_t>(r.stride()), K = static_cast<size_t>(r.k);
    const DecodeCheckGroup& g = r.t.c.groups[0];
    auto* in = reinterpret_cast<const uint8_t**>(h + C.in_tab_off);
    auto* pat = reinterpret_cast<uint32_t*>(h + C.pat_off);
    auto* out = reinterpret_cast<uint8_t**>(h + C.out_tab_off[0]);
    auto* fix = reinterpret_cast<uint8_t**>(h + o.fixtab);
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const ItemLayout& il = C.items[j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      pat[j] = pattern(C, j);
      const DecodeCheckPattern& p = r.t.c.patterns[pat[j]];
      for (size_t q = 0; q < stride; ++q)
        in[j * stride + q] = q < p.delivered.size() ? d + il.in_off + il.pitch * q : nullptr;
      for (size_t q = 0; q < p.delivered.size(); ++q)
        segs.push_back({h + il.in_off + il.pitch * q, in_of(id, p.delivered[q]) + it.off, it.w});
      if (!r.store)
        for (size_t q = 0; q < p.rows.size(); ++q)
          segs.push_back({h + il.out_off + il.pitch * q, dst_of(id, p.rows[q]) + it.off, it.w});
      for (int row = 0; row < g.R; ++row)
        out[j * static_cast<size_t>(g.R) + row] =
            row < static_cast<int>(g.nrows[pat[j]]) ? d + il.out_off + il.pitch * static_cast<size_t>(row) : nullptr;
      for (size_t q = 0; q < fix_slots(r.k); ++q) {
        const size_t nfix = K + r.t.nchk[pat[j]];
        const int shard = q < K ? p.expect[q] : q < nfix ? p.rows[q - K] : -1;
        fix[j * fix_slots(r.k) + q] = shard >= 0 && fix_of(id, shard) ? d + o.item[j] + il.pitch * q : nullptr;
      }
    }
    fill_chunk_tile_map(C, items, h);
    std::memset(h + C.status_off, 0, sizeof(int) * C.count);
    return RS_OK;
  }

  int send(Slot& sl, const ChunkLayout& C) {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const RepairOffsets o = offsets(C);
    const uint8_t* tabs = static_cast<const uint8_t*>(L.rag_tabs.p);
    const DecodeCheckGroup& g = r.t.c.groups[0];
    const size_t rows0 = C.items[0].out_off;
    HIPCHK(hipMemcpyAsync(d, h, C.status_off + sizeof(int) * C.count, hipMemcpyHostToDevice, sl.stream));
    if (!r.store)
      HIPCHK(hipMemcpyAsync(d + rows0, h + rows0, C.out_end - rows0, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(hipMemcpyAsync(d + o.fixtab, h + o.fixtab, o.counts - o.fixtab, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(hipMemsetAsync(d + o.counts, 0, o.total - o.counts, sl.stream));  // the counts and every fix row
    RepairArgs x{};
    UpdateArgs& u = x.c.m.u;
    const ApplyArgs a = chunk_launch_args(C, d, 0, r.stride(), g.R, tabs + tab_off[1], g.tab_stride, u);
    u.nsrc = reinterpret_cast<const uint32_t*>(tabs + tab_off[0]);
    u.in_stride = static_cast<uint32_t>(r.stride());
    x.c.m.nrows = reinterpret_cast<const uint32_t*>(tabs + tab_off[2]);
    x.c.cmask = reinterpret_cast<const uint32_t*>(tabs + tab_off[3]);
    x.gf = tabs + tab_off[4];
    x.loc = tabs + tab_off[5];
    x.counts = reinterpret_cast<uint64_t*>(d + o.counts);
    x.fix = reinterpret_cast<uint8_t* const*>(d + o.fixtab);
    x.loc_stride = static_cast<uint32_t>(r.t.stride);
    x.nbins = static_cast<uint32_t>(r.bins());
    x.k = r.k;
    HIPCHK(launch_decode_repair(a, x, r.store, C.any_tail, sl.stream));
    HIPCHK(hipMemcpyAsync(h + C.status_off, d + C.status_off,
                          (any_wanted ? C.out_end : C.status_off + sizeof(int) * C.count) - C.status_off,
                          hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipMemcpyAsync(h + o.counts, d + o.counts, sizeof(uint64_t) * C.count * r.bins(), hipMemcpyDeviceToHost,
                          sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.ctx->n_chunks.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_launches.fetch_add(1, std::memory_order_relaxed);
    r.ctx->n_copies.fetch_add(r.store ? 4 : 5, std::memory_order_relaxed);
    return RS_OK;
  }

  // The wanted rows, the flags and the counts; then the blamed fix rows the caller asked for,
  // while the chunk's device mirror still stands.
  int collect(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = staging(sl);
    const RepairOffsets o = offsets(C);
    const int* st = reinterpret_cast<const int*>(h + C.status_off);
    const uint64_t* cn = reinterpret_cast<const uint64_t*>(h + o.counts);
    const size_t K = static_cast<size_t>(r.k), nb = r.bins();
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      const uint32_t pi = pattern(C, j);
      const DecodeCheckPattern& p = r.t.c.patterns[pi];
      if (st[j]) flags[id] = 1;
      for (size_t q = 0; q < nb; ++q) counts[static_cast<size_t>(id) * nb + q] += cn[j * nb + q];
      for (size_t q = r.t.nchk[pi]; q < p.rows.size(); ++q)
        segs.push_back({dst_of(id, p.rows[q]) + it.off, h + C.items[j].out_off + C.items[j].pitch * q, it.w});
      for (size_t q = 0; q < K + r.t.nchk[pi]; ++q) {
        const int shard = q < K ? p.expect[q] : p.rows[q - K];
        uint8_t* to = fix_of(id, shard);
        if (!to || cn[j * nb + static_cast<size_t>(shard)] == 0) continue;
        row.resize(it.w);
        HIPCHK(hipMemcpy(row.data(), base(sl) + o.item[j] + C.items[j].pitch * q, it.w, hipMemcpyDeviceToHost));
        r.ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
        for (size_t c = 0; c < it.w; ++c) to[it.off + c] ^= row[c];
      }
    }
    return RS_OK;
  }
};

// The call's runnable stripes `ids` (each is in the launch, with a nonzero size, k expected
// shards and at most 16 rows) on one device and lane. flags: batch * (k + m) bytes of the whole
// call, bit 0 expected, bit 1 delivered, bit 2 wanted, bit 3 compared, bit 4 a fix buffer given.
// counts: the call's, zeroed by the caller; corrupt: per stripe, set where a column mismatched.
template <class InF, class DstF, class FixF>
int run_decode_repair(rs_ctx* ctx, int k, int m, bool store, const std::vector<int>& ids, const size_t* sizes,
                      const uint8_t* flags, InF in_of, DstF dst_of, FixF fix_of, uint64_t* counts, int* corrupt) {
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
  const size_t per = pattern_arena_bytes(k, kRepairRows) + locate_stride(k);
  return with_lane(ctx, dev, [&](Lane& L) -> int {
    HIPCHK(hipSetDevice(dev->id));
    return for_each_run(ids, n, per, fl.data(), [&](size_t begin, size_t end) -> int {
      DecodeRepairRun r{ctx, k, m, store, {}, {}, {}};
      r.ids.assign(ids.begin() + static_cast<ptrdiff_t>(begin), ids.begin() + static_cast<ptrdiff_t>(end));
      const std::vector<size_t> rsz(sz.begin() + static_cast<ptrdiff_t>(begin), sz.begin() + static_cast<ptrdiff_t>(end));
      const size_t cells = (end - begin) * n;
      std::vector<uint8_t> ex(cells), hin(cells), hdst(cells), hchk(cells), hfix(cells);
      for (size_t i = 0; i < cells; ++i) {
        const uint8_t f = fl[begin * n + i];
        ex[i] = f & 1u;
        hin[i] = (f >> 1) & 1u;
        hdst[i] = (f >> 2) & 1u;
        hchk[i] = (f >> 3) & 1u;
        hfix[i] = (f >> 4) & 1u;
      }
      const DecodeRepairError te = build_decode_repair_tables(k, m, static_cast<int>(end - begin), rsz.data(), ex.data(),
                                                              hin.data(), hdst.data(), hchk.data(), hfix.data(), r.t);
      if (te == DecodeRepairError::kSingular) return RS_E_SINGULAR;
      if (te != DecodeRepairError::kOk || r.t.c.groups.size() != 1) return RS_E_ARG;
      r.sh = ragged_shape(r.stride(), r.t.c.groups, rsz, [&](int s) {
        const uint32_t p = r.t.c.pat[static_cast<size_t>(s)];
        return std::make_pair(static_cast<int>(r.t.c.nsrc[p]), static_cast<int>(r.t.c.nrows[p]));
      });
      RaggedWork w(r.sh, chunk_bytes());
      if (!w.cut(r.sh, chunk_bytes())) return RS_E_ARG;
      DecodeRepairJob<InF, DstF, FixF> job(r, L, w.items, in_of, dst_of, fix_of, counts, corrupt);
      return run_chunk_pipeline(ctx, L, w.chunks, job);
    });
  });
}

}  // namespace
}  // namespace callfs
