// The one chunk pipeline of the tile-map routes of the host-memory path:
// the ragged batches (host_ragged.hpp), update (host_update.hpp) and locate / correct
// (host_locate.hpp) all send their chunks (ragged_chunks.hpp) through run_chunk_pipeline, which
// owns the slot rotation; a route is a job that says what a chunk needs, stages, sends and
// yields. Beside it what those jobs share: the staged transport's slots, a lane's table upload
// and a chunk's launch arguments. Included by rs_host.cpp only.
#pragma once

#include "host_common.hpp"
#include "ragged_chunks.hpp"

namespace callfs {
namespace {

// Sends `chunks` through the lane's slots, chunk c on slot c % nslots. A job supplies
//   prepare_run()          the run's tables on the lane
//   staging_bytes(C)       the staging chunk C needs
//   prepare(sl, bytes)     a slot's buffers for the largest chunk
//   stage(sl, C, segs)     C's metadata into the slot's staging, and in `segs` its copy-in
//   send(sl, C)            the copies and launches, ending in what wait() waits for
//   wait(sl)               until the chunk the slot holds has landed in its staging
//   collect(sl, C, segs)   its flags and counts, and in `segs` its copy-out
//   landed()               once that copy-out has run
// The rows of the chunk a slot held before are copied out before the new chunk is staged: chunks
// of one run are laid out differently, so its inputs may lie where those outputs were. The last
// chunks drain in order. sl.pending and sl.rag_chunk are with_lane's to read on an error.
template <class Job>
int run_chunk_pipeline(rs_ctx* ctx, Lane& L, const std::vector<ChunkLayout>& chunks, Job& job) {
  int rc;
  if ((rc = job.prepare_run())) return rc;
  size_t bytes = 0;
  for (const ChunkLayout& C : chunks) bytes = std::max(bytes, job.staging_bytes(C));
  const size_t nchunks = chunks.size();
  const size_t nslots = std::min<size_t>(nchunks, static_cast<size_t>(pipeline_slots()));
  for (size_t si = 0; si < nslots; ++si) {
    if ((rc = job.prepare(L.slot[si], bytes))) return rc;
    L.slot[si].pending = false;
  }
  std::vector<CopyPool::Seg> segs;
  auto copy = [&] {
    if (!segs.empty()) ctx->pool.run(segs);
    segs.clear();
  };
  auto drain = [&](Slot& sl) -> int {
    if (!sl.pending) return RS_OK;
    int drc;
    if ((drc = job.wait(sl)) || (drc = job.collect(sl, chunks[sl.rag_chunk], segs))) return drc;
    sl.pending = false;
    copy();
    return job.landed();
  };
  for (size_t c = 0; c < nchunks; ++c) {
    Slot& sl = L.slot[c % nslots];
    if ((rc = drain(sl)) || (rc = job.stage(sl, chunks[c], segs))) return rc;
    copy();
    if ((rc = job.send(sl, chunks[c]))) return rc;
    sl.pending = true;
    sl.rag_chunk = c;
  }
  for (size_t c = nchunks - nslots; c < nchunks; ++c)
    if ((rc = drain(L.slot[c % nslots]))) return rc;
  return RS_OK;
}

// The slots of the staged transport: pinned staging and its device mirror at the same offsets,
// and the slot's event, recorded behind a chunk's D2H.
struct StagedSlots {
  int prepare(Slot& sl, size_t bytes) {
    if (const int rc = sl.dev.ensure(bytes)) return rc;
    return sl.host.ensure(bytes);
  }
  uint8_t* staging(Slot& sl) const { return static_cast<uint8_t*>(sl.host.p); }
  uint8_t* base(Slot& sl) const { return static_cast<uint8_t*>(sl.dev.p); }
  int wait(Slot& sl) const {
    HIPCHK(hipEventSynchronize(sl.done));
    return RS_OK;
  }
  int landed() { return RS_OK; }
};

// A run's tables in a lane's device buffer `buf`: the pieces packed in order (off[i]: piece i's
// offset), uploaded unless `key_slot` says the buffer holds them already. A piece without bytes
// of its own is zeroed, and fill(h) writes it into the host image before the upload.
struct TablePiece {
  const void* p;
  size_t bytes;
};
template <class Fill>
int upload_lane_tables(rs_ctx* ctx, DevBuf& buf, std::string& key_slot, std::string key,
                       const std::vector<TablePiece>& pieces, std::vector<size_t>& off, Fill fill) {
  Packer pk;
  off.clear();
  for (const TablePiece& t : pieces) off.push_back(pk.take(t.bytes));
  if (buf.p && key_slot == key) return RS_OK;
  key_slot.clear();
  if (const int rc = buf.ensure(pk.off)) return rc;
  std::vector<uint8_t> h(pk.off, 0);
  for (size_t i = 0; i < pieces.size(); ++i)
    if (pieces[i].p) std::memcpy(h.data() + off[i], pieces[i].p, pieces[i].bytes);
  fill(h.data());
  HIPCHK(hipMemcpy(buf.p, h.data(), h.size(), hipMemcpyHostToDevice));
  ctx->n_copies.fetch_add(1, std::memory_order_relaxed);
  key_slot = std::move(key);
  return RS_OK;
}
inline int upload_lane_tables(rs_ctx* ctx, DevBuf& buf, std::string& key_slot, std::string key,
                              const std::vector<TablePiece>& pieces, std::vector<size_t>& off) {
  return upload_lane_tables(ctx, buf, key_slot, std::move(key), pieces, off, [](uint8_t*) {});
}

// The launch arguments of launch group gi (R rows, tables at `tabs`, `tab_stride` apart) over
// the chunk laid out by C at `base` (device-visible): the pointer tables and status words in
// the result, the tile-map pointers in x (RaggedArgs or UpdateArgs).
template <class X>
ApplyArgs chunk_launch_args(const ChunkLayout& C, uint8_t* base, size_t gi, int K, int R, const uint8_t* tabs,
                            size_t tab_stride, X& x) {
  ApplyArgs a{};
  a.in_tab = reinterpret_cast<const uint8_t* const*>(base + C.in_tab_off);
  a.out_tab = reinterpret_cast<uint8_t* const*>(base + C.out_tab_off[gi]);
  a.ltabs = tabs;
  a.status = reinterpret_cast<int*>(base + C.status_off);
  a.status_stride = 1;
  a.K = K;
  a.R = R;
  a.batch = static_cast<int>(C.count);
  x.pat = reinterpret_cast<const uint32_t*>(base + C.pat_off);
  x.size = reinterpret_cast<const uint64_t*>(base + C.size_off);
  x.tile0 = reinterpret_cast<const uint32_t*>(base + C.tile0_off);
  x.tile_stripe = reinterpret_cast<const uint32_t*>(base + C.tile_stripe_off);
  x.tab_stride = static_cast<uint32_t>(tab_stride);
  x.ntiles = C.ntiles;
  return a;
}

// The split of a call's runnable stripes `ids` into runs (ragged_segments): flag row j is stripe
// ids[j]'s, `width` bytes, and a pattern costs `per` bytes of tables. fn(begin, end) runs
// ids[begin, end).
template <class F>
int for_each_run(const std::vector<int>& ids, size_t width, size_t per, const uint8_t* rows, F fn) {
  std::vector<int> all(ids.size());
  for (size_t j = 0; j < all.size(); ++j) all[j] = static_cast<int>(j);
  for (const auto& seg : ragged_segments(width, per, all, rows, kRaggedArenaBudget))
    if (const int rc = fn(seg.first, seg.second)) return rc;
  return RS_OK;
}

}  // namespace
}  // namespace callfs
