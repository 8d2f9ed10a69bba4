// The ragged pipeline of the host-memory path: a batch call whose runnable
// stripes differ in shard size or erasure pattern runs as one pipeline over items
// (ragged_chunks.hpp) instead of one uniform pipeline per (S, flag row) group. A stripe's flag
// row (host_path.hpp kShard*) says which shards are present, wanted or left alone; a call
// without a wanted set is the all-wanted case of the same code. It owns the runs of
// a call (RaggedRun), their pattern tables on a lane, the staged, in-place and direct
// transports, the ragged job of the one chunk pipeline (RaggedJob; host_chunks.hpp has the
// slot rotation) and run_ragged, which picks the device and the lane. Included by rs_host.cpp
// only.
#pragma once

#include "host_chunks.hpp"
#include "sha256.hpp"

namespace callfs {
namespace {

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
  // a checksummed codec batch, else null; sums_host[s] = 1: stripe s of the
  // run hashes on the host (sums_route)
  const SumsCall* sums = nullptr;
  std::vector<uint8_t> sums_host;
  const Join* join_of(int id) const { return joins ? joins + id : nullptr; }
  const MixedPattern& pattern(int s) const { return mt.patterns[mt.pat[static_cast<size_t>(s)]]; }
  void count(size_t chunks, size_t copies) const {
    ctx->n_chunks.fetch_add(chunks, std::memory_order_relaxed);
    ctx->n_launches.fetch_add(chunks * mt.groups.size(), std::memory_order_relaxed);
    ctx->n_copies.fetch_add(copies, std::memory_order_relaxed);
  }
};

// What a lane's table cache is keyed by: the profile, the rows per pattern and the patterns
// (one mask has as many patterns as wanted sets: their rows tell them apart).
std::string ragged_key(const RaggedRun& r) {
  std::string key = std::to_string(r.k) + "," + std::to_string(r.m) + "," + std::to_string(r.mt.rows) + ":";
  for (const MixedPattern& p : r.mt.patterns) key.append(reinterpret_cast<const char*>(p.mask.data()), p.mask.size());
  for (const MixedPattern& p : r.mt.patterns) {
    key.push_back('|');
    for (int i : p.rows) key.push_back(static_cast<char>(i));
  }
  return key;
}

// The run's compare masks and nibble-table arenas in the lane's device buffer, per launch group
// [vmask][arena] (off[2 * gi], off[2 * gi + 1]); uploaded when the lane last held another run's.
int upload_ragged_tables(const RaggedRun& r, Lane& L, std::vector<size_t>& off) {
  std::vector<TablePiece> pieces;
  for (const MixedGroup& g : r.mt.groups) {
    pieces.push_back({g.vmask.data(), sizeof(uint32_t) * g.vmask.size()});
    pieces.push_back({g.arena.data(), g.arena.size()});
  }
  return upload_lane_tables(r.ctx, L.rag_tabs, L.rag_key, ragged_key(r), pieces, off);
}

// launch_ragged of every launch group over the chunk laid out by C at `base` (device-visible).
hipError_t launch_ragged_chunk(const RaggedRun& r, const ChunkLayout& C, uint8_t* base,
                               const uint8_t* tabs, const std::vector<size_t>& off, hipStream_t s) {
  for (size_t gi = 0; gi < r.mt.groups.size(); ++gi) {
    const MixedGroup& g = r.mt.groups[gi];
    RaggedArgs x{};
    const ApplyArgs a = chunk_launch_args(C, base, gi, r.k, g.R, tabs + off[2 * gi + 1], g.tab_stride, x);
    x.vmask = reinterpret_cast<const uint32_t*>(tabs + off[2 * gi]);
    const hipError_t e = launch_ragged(a, x, nullptr, C.any_tail, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Staged: one H2D of the chunk's input region (through the zeroed status words that open the
// output region), launch_ragged per launch group on the slot's device mirror, the hash launch
// of a chunk that carries a message table (sha256_rows over the rows where they lie), one D2H
// of the output region, then the slot's event.
struct RaggedStaged : StagedSlots {
  const RaggedRun& r;
  Lane& L;
  std::vector<size_t> tab_off;
  RaggedStaged(const RaggedRun& run, Lane& lane) : r(run), L(lane) {}
  int prepare_run() { return upload_ragged_tables(r, L, tab_off); }
  int send(Slot& sl, const ChunkLayout& C) const {
    uint8_t* h = staging(sl);
    uint8_t* d = base(sl);
    const size_t head = C.status_off + sizeof(int) * C.count;
    HIPCHK(hipMemcpyAsync(d, h, head, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(launch_ragged_chunk(r, C, d, static_cast<const uint8_t*>(L.rag_tabs.p), tab_off, sl.stream));
    if (C.sums_count) {
      Sha256RowsArgs a{};
      a.base = d;
      a.table = reinterpret_cast<const uint32_t*>(d + C.sums_tab_off);
      a.expected = C.sums == SumsMode::kCheck ? reinterpret_cast<const uint32_t*>(d + C.sums_expect_off) : nullptr;
      a.out = d + C.sums_out_off;
      a.count = static_cast<uint32_t>(C.sums_count);
      HIPCHK(launch_sha256_rows(a, sl.stream));
      r.ctx->n_launches.fetch_add(1, std::memory_order_relaxed);
    }
    HIPCHK(hipMemcpyAsync(h + C.status_off, d + C.status_off, C.out_end - C.status_off,
                          hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipEventRecord(sl.done, sl.stream));
    r.count(1, 2);
    return RS_OK;
  }
};

// In place: rs_apply_small_ragged on host-coherent staging, one dispatch per launch group;
// the host spins on the completion flag the last group releases (host_common.hpp). The
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
    std::vector<TablePiece> pieces;  // built by the fill below, on an upload alone
    for (const MixedGroup& g : r.mt.groups) {
      pstride.push_back(4u + static_cast<uint32_t>(r.k) * g.R * kTabWords);
      pieces.push_back({nullptr, sizeof(uint32_t) * pstride.back() * P});
    }
    return upload_lane_tables(r.ctx, L.rag_small_tabs, L.rag_small_key, ragged_key(r), pieces, tab_off, [&](uint8_t* h) {
      for (size_t gi = 0; gi < r.mt.groups.size(); ++gi) {
        const MixedGroup& g = r.mt.groups[gi];
        const size_t W = static_cast<size_t>(nibble_width(g.R));
        for (size_t p = 0; p < P; ++p) {
          auto* blk = reinterpret_cast<uint32_t*>(h + tab_off[gi]) + p * pstride[gi];
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
    });
  }
  int prepare(Slot& sl, size_t bytes) {
    done_off = round_up(bytes, 256);
    return done_flag_ensure(sl, done_off);
  }
  uint8_t* staging(Slot& sl) const { return static_cast<uint8_t*>(sl.small.p); }
  uint8_t* base(Slot& sl) const { return staging(sl); }
  int send(Slot& sl, const ChunkLayout& C) const {
    uint8_t* b = staging(sl);
    int* done = done_flag_arm(sl, done_off);
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
  int wait(Slot& sl) const { return done_flag_wait(sl, done_off); }
  // what the kernel's 32-bit item table can address
  static bool fits(const ChunkLayout& C) {
    if (C.out_end >= (1ull << 35) || C.count > kRaggedMaxItems) return false;
    for (const ItemLayout& it : C.items)
      if (it.pitch > 0xFFFFFFF0u) return false;
    return true;
  }
};

// The ragged job of the chunk pipeline (host_chunks.hpp): per chunk the metadata is written and
// the input rows are copied into the slot's staging, the transport sends it, and the output rows
// come out of the staging when the chunk has landed. in / out take a stripe of the call's
// runnable list and a shard index; flags (per runnable stripe) receive 1 where a compared row
// mismatched.
// A checksummed codec batch (r.sums): a chunk with a message table gets it and -- a decode --
// its slots' expected digests written beside the metadata, and its digests or flags are read
// when it drains. The host-hashed stripes of a decode are hashed before the chunk that holds
// their first item is staged, those of an encode once the chunk that holds their last item has
// drained and its rows have landed in the caller's buffers. A decode delivers nothing of a
// stripe with a mismatch (the caller runs it again): the join of a device-checked item's
// present data shards therefore waits for the chunk's flags and is copied from its staging.
template <class Transport, class InF, class OutF>
struct RaggedJob {
  const RaggedRun& r;
  const std::vector<RaggedItem>& items;
  Transport& tr;
  InF& in;
  OutF& out;
  int* flags;
  const size_t k = static_cast<size_t>(r.k);
  const SumsCall* sums = r.sums;
  const bool check = sums && sums->mode == SumsMode::kCheck;
  std::vector<SumsTask> tasks;  // host hashes, gathered by collect and stage

  int prepare_run() { return tr.prepare_run(); }
  size_t staging_bytes(const ChunkLayout& C) const { return C.out_end; }
  int prepare(Slot& sl, size_t bytes) { return tr.prepare(sl, bytes); }
  int send(Slot& sl, const ChunkLayout& C) { return tr.send(sl, C); }
  int wait(Slot& sl) { return tr.wait(sl); }
  // an encode's host-hashed stripes that just completed: their rows are in the caller's buffers
  int landed() { return run_tasks(); }
  int run_tasks() {
    run_sums_tasks(r.ctx->pool, tasks);
    tasks.clear();
    return RS_OK;
  }

  // the shards of stripe s that are hashed, by the pattern: valid[], the compared rows and
  // (an encode) the written rows
  template <class F>
  void hashed_shards(int s, F&& fn) const {
    const MixedPattern& pt = r.pattern(s);
    for (int i : pt.valid) fn(i);
    for (size_t row = 0; row < pt.rows.size(); ++row)
      if (!check || row >= static_cast<size_t>(pt.missing)) fn(pt.rows[row]);
  }
  bool stripe_bad(int s) const {
    bool any = false;
    hashed_shards(s, [&](int i) { any |= sums->bad[sums->at(r.ids[static_cast<size_t>(s)], i)] != 0; });
    return any;
  }
  bool on_host(int s) const { return sums && r.sums_host[static_cast<size_t>(s)]; }

  int collect(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = tr.staging(sl);
    const int* st = reinterpret_cast<const int*>(h + C.status_off);
    if (C.sums_count) {
      const std::vector<SumsSlot> slots = sums_slots(C, r.sh, items, r.mt);
      for (size_t s = 0; s < slots.size(); ++s) {
        const size_t at = sums->at(r.ids[static_cast<size_t>(slots[s].stripe)], slots[s].shard);
        if (check) sums->bad[at] = h[C.sums_out_off + s] != 0;
        else std::memcpy(sums->digests + 32 * at, h + C.sums_out_off + 32 * s, 32);
      }
    }
    for (size_t j = 0; j < C.count; ++j) {
      const RaggedItem& it = items[C.first + j];
      const int id = r.ids[static_cast<size_t>(it.stripe)];
      if (check && stripe_bad(it.stripe)) continue;  // nothing of it is delivered
      if (st[j]) flags[id] = 1;
      const MixedPattern& pt = r.pattern(it.stripe);
      if (sums && !check && on_host(it.stripe) && it.off + it.w == r.sh.size[static_cast<size_t>(it.stripe)])
        hashed_shards(it.stripe, [&](int i) {
          tasks.push_back(sums_task(*sums, id, i, out(id, i), r.sh.size[static_cast<size_t>(it.stripe)]));
        });
      // the join a device-checked item held back: its present data shards, from staging
      for (size_t i = 0; check && !on_host(it.stripe) && i < k; ++i) {
        const auto js = join_span(r.join_of(id), pt.valid[i], it.off, it.w);
        if (js.first) segs.push_back({js.first, h + C.items[j].in_off + C.items[j].pitch * i, js.second});
      }
      for (int row = 0; row < pt.missing; ++row) {
        const int i = pt.rows[static_cast<size_t>(row)];
        const auto tee = join_span(r.join_of(id), i, it.off, it.w);
        segs.push_back({out(id, i) + it.off,
                        h + C.items[j].out_off + C.items[j].pitch * static_cast<size_t>(row), it.w,
                        tee.first, tee.second});
      }
    }
    return RS_OK;
  }

  int stage(Slot& sl, const ChunkLayout& C, std::vector<CopyPool::Seg>& segs) {
    uint8_t* h = tr.staging(sl);
    uint8_t* b = tr.base(sl);
    if (check) {
      for (size_t j = 0; j < C.count; ++j) {
        const RaggedItem& it = items[C.first + j];
        if (!on_host(it.stripe) || it.off) continue;
        const int id = r.ids[static_cast<size_t>(it.stripe)];
        hashed_shards(it.stripe, [&](int i) {
          tasks.push_back(sums_task(*sums, id, i, in(id, i), r.sh.size[static_cast<size_t>(it.stripe)]));
        });
      }
      run_tasks();
    }
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
      // a checked decode joins no shard before its stripe's flags are known
      const bool tee_now = !check || (on_host(it.stripe) && !stripe_bad(it.stripe));
      for (size_t i = 0; i < k; ++i) {
        const auto tee = join_span(tee_now ? r.join_of(id) : nullptr, pt.valid[i], it.off, it.w);
        segs.push_back({h + C.items[j].in_off + C.items[j].pitch * i, in(id, pt.valid[i]) + it.off, it.w,
                        tee.first, tee.second});
      }
      for (size_t row = static_cast<size_t>(pt.missing); row < pt.rows.size(); ++row)
        segs.push_back({row_at(h, j, static_cast<int>(row)), in(id, pt.rows[row]) + it.off, it.w});
    }
    if (C.sums_count) {
      const std::vector<SumsSlot> slots = sums_slots(C, r.sh, items, r.mt);
      sums_fill_table(slots, reinterpret_cast<uint32_t*>(h + C.sums_tab_off));
      for (size_t s = 0; check && s < slots.size(); ++s)
        std::memcpy(h + C.sums_expect_off + 32 * s,
                    sums->expected + 32 * sums->at(r.ids[static_cast<size_t>(slots[s].stripe)], slots[s].shard), 32);
    }
    return RS_OK;
  }
};

template <class Transport, class InF, class OutF>
int run_ragged_chunks(const RaggedRun& r, Lane& L, const std::vector<RaggedItem>& items,
                      const std::vector<ChunkLayout>& chunks, Transport& tr, InF& in, OutF& out,
                      int* flags) {
  RaggedJob<Transport, InF, OutF> job{r, items, tr, in, out, flags};
  return run_chunk_pipeline(r.ctx, L, chunks, job);
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
  std::vector<size_t> tab_off;
  int rc;
  if ((rc = upload_ragged_tables(r, L, tab_off))) return rc;
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
  HIPCHK(launch_ragged_chunk(r, C, d, static_cast<const uint8_t*>(L.rag_tabs.p), tab_off, sl.stream));
  if (compares)
    HIPCHK(hipMemcpyAsync(sl.hstat.p, d + C.status_off, sizeof(int) * C.count, hipMemcpyDeviceToHost,
                          sl.stream));
  HIPCHK(hipEventRecord(sl.done, sl.stream));
  r.count(1, compares ? 2 : 1);
  std::vector<CopyPool::Seg> present, rebuilt;
  for (size_t j = 0; r.joins && j < C.count; ++j) {
    const int id = r.ids[j];
    const MixedPattern& pt = r.pattern(static_cast<int>(j));
    const size_t S = r.sh.size[j];
    for (int i : pt.valid) {
      const auto js = join_span(r.join_of(id), i, 0, S);
      if (js.first) present.push_back({js.first, in(id, i), js.second});
    }
    for (int row = 0; row < pt.missing; ++row) {
      const int i = pt.rows[static_cast<size_t>(row)];
      const auto js = join_span(r.join_of(id), i, 0, S);
      if (js.first) rebuilt.push_back({js.first, out(id, i), js.second});
    }
  }
  if ((rc = join_around_launch(r.ctx, sl, present, rebuilt))) return rc;
  if (compares) {
    const int* st = static_cast<const int*>(sl.hstat.p);
    for (size_t j = 0; j < C.count; ++j)
      if (st[j]) flags[r.ids[j]] = 1;
  }
  return RS_OK;
}

// A heterogeneous batch call on one device and lane. The call's runnable stripes are listed
// by S[j] and the kShard* flags (host_path.hpp) present[j * n ..]; in(j, i) / out(j, i) give
// runnable stripe j's shard i. An unwanted missing shard is neither read nor
// written. The stripes run in classes by row count (ragged_classes). by_missing: a reconstruct
// without verification, whose patterns' rows are their wanted missing shards alone (the
// compared rows are dropped). flags[j] = 1 where stripe j's compared rows mismatched.
template <class InF, class OutF>
int run_ragged_on_lane(rs_ctx* ctx, Lane& L, int device, int k, int m, bool by_missing,
                       const std::vector<size_t>& S, const std::vector<uint8_t>& present, InF& in,
                       OutF& out, int* flags, const Join* joins, const SumsCall* sums) {
  HIPCHK(hipSetDevice(device));
  const int n = k + m, stripes = static_cast<int>(S.size());
  const size_t nn = static_cast<size_t>(n);
  // direct: every buffer pinned, and the call at or above the zero-copy threshold
  unsigned long long total = 0;
  for (size_t s : S) total += static_cast<unsigned long long>(s) * nn;
  // (a checksummed batch takes the staged transport alone)
  bool direct = !sums && !ctx->pinned.empty() && total >= zero_copy_min(nn);
  for (int j = 0; direct && j < stripes; ++j)
    for (int i = 0; direct && i < n; ++i) {
      const bool written = present[static_cast<size_t>(j) * nn + i] == kShardWanted;
      if (present[static_cast<size_t>(j) * nn + i] == kShardUnwanted) continue;
      if (by_missing && !written) {
        // only the first k present shards are read
        int before = 0;
        for (int q = 0; q < i; ++q) before += present[static_cast<size_t>(j) * nn + q] == kShardPresent;
        if (before >= k) continue;
      }
      direct = ctx->pinned.contains(written ? out(j, i) : in(j, i), S[static_cast<size_t>(j)]);
    }
  for (int j = 0; direct && joins && j < stripes; ++j)
    direct = joins[j].len == 0 || ctx->pinned.contains(joins[j].out, joins[j].len);
  for (const RaggedClass& cls : ragged_classes(n, k, stripes, present.data(), !by_missing)) {
    for (const auto& seg : ragged_segments(k, n, cls.rows, cls.stripes, present.data(), kRaggedArenaBudget)) {
      RaggedRun r{ctx, k, m, {}, {}, {}, joins, sums, {}};
      r.ids.assign(cls.stripes.begin() + static_cast<ptrdiff_t>(seg.first),
                   cls.stripes.begin() + static_cast<ptrdiff_t>(seg.second));
      std::vector<uint8_t> pres(r.ids.size() * nn), want(pres.size());
      for (size_t s = 0; s < r.ids.size(); ++s)
        shard_flags_split(&present[static_cast<size_t>(r.ids[s]) * nn], nn, &pres[s * nn], &want[s * nn]);
      const int count = static_cast<int>(r.ids.size());
      const TableError me = build_mixed_tables(k, m, count, pres.data(), want.data(), r.mt, !by_missing);
      if (me == TableError::kSingular) return RS_E_SINGULAR;
      // every pattern of the class has its rows: the tables are what the kernels expect
      if (me != TableError::kOk || !mixed_rows_are(r.mt, cls.rows)) return RS_E_ARG;
      std::vector<size_t> sizes(r.ids.size());
      for (size_t s = 0; s < sizes.size(); ++s) sizes[s] = S[static_cast<size_t>(r.ids[s])];
      r.sh = ragged_shape(k, r.mt.groups, std::move(sizes), [&](int s) {
        const MixedPattern& pt = r.pattern(s);
        return std::make_pair(k + static_cast<int>(pt.rows.size()) - pt.missing, pt.missing);
      });
      int rc;
      if (direct) {
        if ((rc = run_ragged_direct(r, L, in, out, flags))) return rc;
        continue;
      }
      RaggedWork w(r.sh, chunk_bytes());
      if (sums) {
        // packed with the regions of the hash launch; the rule then takes them out of the
        // chunks that hash on the host
        const SumsKnob knob = sums_device_knob();
        if (!w.cut(r.sh, chunk_bytes(), knob == SumsKnob::kHost ? SumsMode::kNone : sums->mode)) return RS_E_ARG;
        r.sums_host = sums_route(r.sh, w.items, w.chunks, knob);
        RaggedStaged tr(r, L);
        if ((rc = run_ragged_chunks(r, L, w.items, w.chunks, tr, in, out, flags))) return rc;
        continue;
      }
      // the whole run as one in-place chunk on slot 0
      if (w.items.size() <= kRaggedMaxItems && small_max_bytes() > 0) {
        std::vector<ChunkLayout> one(1, layout_chunk(r.sh, w.items, 0, w.items.size()));
        if (one[0].out_end <= small_max_bytes() && RaggedInplace::fits(one[0])) {
          RaggedInplace tr{r, L, {}, {}, 0};
          if ((rc = run_ragged_chunks(r, L, w.items, one, tr, in, out, flags))) return rc;
          continue;
        }
      }
      if (!w.cut(r.sh, chunk_bytes())) return RS_E_ARG;
      bool inplace = inplace_pipeline();
      for (const ChunkLayout& C : w.chunks) inplace = inplace && RaggedInplace::fits(C);
      if (inplace) {
        RaggedInplace tr{r, L, {}, {}, 0};
        rc = run_ragged_chunks(r, L, w.items, w.chunks, tr, in, out, flags);
      } else {
        RaggedStaged tr(r, L);
        rc = run_ragged_chunks(r, L, w.items, w.chunks, tr, in, out, flags);
      }
      if (rc) return rc;
    }
  }
  return RS_OK;
}

template <class InF, class OutF>
int run_ragged(rs_ctx* ctx, int k, int m, bool by_missing, const std::vector<size_t>& S,
               const std::vector<uint8_t>& present, InF in, OutF out, int* flags,
               const Join* joins = nullptr, const SumsCall* sums = nullptr) {
  if (ctx->devs.empty()) return RS_E_HIP;
  ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  ctx->n_ragged_calls.fetch_add(1, std::memory_order_relaxed);
  // one device and lane, chosen round-robin like any call (split_ways does not apply)
  Device* dev = ctx->devs[device_slot(ctx->rr.fetch_add(1), 0, ctx->devs.size())].get();
  return with_lane(ctx, dev, [&](Lane& L) {
    return run_ragged_on_lane(ctx, L, dev->id, k, m, by_missing, S, present, in, out, flags, joins, sums);
  });
}

}  // namespace
}  // namespace callfs
