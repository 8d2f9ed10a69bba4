// Decode sessions of the C ABI (include/callfs_rs.h): the host route over a feed
// object. A session keeps one stripe's rows -- the syndrome accumulators of the compared shards,
// then the wanted shards -- resident on one device from open to close; every arrival is one
// rs_feed launch on the session's stream, from a slot of a small ring of source buffers, and
// finish closes the decode with one final decode-check or decode-repair plan over the resident
// rows with nothing delivered. Built on rs_plan.cpp's public calls alone; a session holds no Lane.
#include <mutex>

#include "host_session.hpp"
#include "rs_internal.hpp"

using namespace callfs;

struct rs_session {
  rs_ctx* ctx = nullptr;
  int device = 0;
  int k = 0, m = 0;
  size_t S = 0, pitch = 0;
  bool repair = false;
  size_t inplace_max = 0;
  std::mutex mu;
  SessionBook book;
  std::vector<int> rows;  // compared ascending, then wanted ascending: row r at rowbuf + r * pitch
  size_t ncmp = 0;
  DevBuf rowbuf;
  HostBuf out;  // the wanted rows' span on its way to pageable destinations
  rs_feed* feed = nullptr;
  hipStream_t stream = nullptr;
  // one source slot: the shard in host-coherent memory the kernel reads in place, or in staging
  // on its way into the device slot; `done` is recorded behind the launch that reads it
  struct Source {
    CoherentBuf coherent;
    HostBuf staging;
    DevBuf dev;
    hipEvent_t done = nullptr;
    bool busy = false;
  };
  Source ring[kSessionMaxSlots];
  size_t depth = 1, next = 0;

  uint8_t* row(int idx) const {
    for (size_t r = 0; r < rows.size(); ++r)
      if (rows[r] == idx) return static_cast<uint8_t*>(rowbuf.p) + r * pitch;
    return nullptr;
  }
  ~rs_session() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (feed) rs_feed_destroy(feed);
    for (Source& s : ring)
      if (s.done) (void)hipEventDestroy(s.done);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

void count(rs_ctx* ctx, uint64_t launches, uint64_t copies) {
  ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  ctx->n_launches.fetch_add(launches, std::memory_order_relaxed);
  ctx->n_copies.fetch_add(copies, std::memory_order_relaxed);
}

// The final plan over the resident rows, launched and read: *corrupt, and the plan's counts in
// repair mode. `fixrow`: per index the device fix row, or null.
int run_final(rs_session& s, const std::vector<int>& delivered, const std::vector<uint8_t*>& fixrow, int* corrupt,
              uint64_t* counts) {
  const size_t n = static_cast<size_t>(s.k + s.m);
  std::vector<const uint8_t*> input(n, nullptr);
  std::vector<uint8_t*> dst(n, nullptr), check(n, nullptr);
  for (int j : delivered) check[static_cast<size_t>(j)] = s.row(j);
  rs_plan* plan = nullptr;
  int rc;
  if (s.repair) {
    for (size_t i = 0; i < n; ++i)
      if (s.book.want[i]) dst[i] = s.row(static_cast<int>(i));
    rc = rs_plan_create_decode_repair(s.ctx, s.device, s.k, s.m, 1, &s.S, s.book.expect.data(), input.data(),
                                      dst.data(), check.data(), fixrow.data(), 0u, &plan);
  } else {
    // the wanted rows are left out: this plan only scans the accumulators
    rc = rs_plan_create_decode_check(s.ctx, s.device, s.k, s.m, 1, &s.S, s.book.expect.data(), input.data(),
                                     dst.data(), check.data(), RS_DECODE_CHECK_FINAL, &plan);
  }
  if (rc) return rc;
  rc = rs_plan_launch(plan, s.stream);
  if (!rc) rc = rs_plan_status(plan, s.stream, corrupt);
  if (!rc && s.repair) rc = rs_plan_blame(plan, s.stream, counts);
  rs_plan_destroy(plan);
  return rc;
}

}  // namespace

extern "C" {

int rs_session_open(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* expect, const uint8_t* want,
                    const uint8_t* compare, unsigned flags, rs_session** out) {
  DeviceGuard dg;
  if (const int rc = check_profile(k, m)) return rc;
  if (!ctx || !expect || !want || !compare || !out || (flags & ~RS_SESSION_REPAIR)) return RS_E_ARG;
  *out = nullptr;
  const int n = k + m;
  FeedTables t;
  switch (build_feed_tables(k, m, S, expect, want, compare, t)) {
    case FeedError::kOk: break;
    case FeedError::kArg: return RS_E_ARG;
    case FeedError::kTooFewShards: return RS_E_TOO_FEW_SHARDS;
    case FeedError::kUnsupported: return RS_E_UNSUPPORTED;
    case FeedError::kNoData: return RS_E_NO_DATA;
    case FeedError::kSingular: return RS_E_SINGULAR;
  }
  if (ctx->devs.empty()) return RS_E_HIP;
  auto s = std::make_unique<rs_session>();
  s->ctx = ctx;
  s->device = ctx->devs[device_slot(ctx->rr.fetch_add(1), 0, ctx->devs.size())]->id;
  s->k = k;
  s->m = m;
  s->S = S;
  s->pitch = round_up(S, kPitchAlign);
  s->repair = (flags & RS_SESSION_REPAIR) != 0;
  s->inplace_max = session_inplace_max();
  s->book.open(k, n, expect, want, compare);
  s->rows = t.rows;
  s->ncmp = t.compared.size();
  HIPCHK(hipSetDevice(s->device));
  int rc;
  if ((rc = s->rowbuf.ensure(std::max<size_t>(1, s->rows.size()) * s->pitch))) return rc;
  HIPCHK(hipMemset(s->rowbuf.p, 0, s->rows.size() * s->pitch));
  if ((rc = s->out.ensure(std::max<size_t>(1, t.wanted.size()) * s->pitch))) return rc;
  HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  s->depth = static_cast<size_t>(session_slots());
  for (size_t q = 0; q < s->depth; ++q) HIPCHK(hipEventCreateWithFlags(&s->ring[q].done, hipEventDisableTiming));
  std::vector<uint8_t*> dst(static_cast<size_t>(n), nullptr), check(static_cast<size_t>(n), nullptr);
  for (int i = 0; i < n; ++i) {
    if (want[i]) dst[static_cast<size_t>(i)] = s->row(i);
    if (compare[i]) check[static_cast<size_t>(i)] = s->row(i);
  }
  if ((rc = rs_feed_create(ctx, s->device, k, m, S, expect, dst.data(), check.data(), &s->feed))) return rc;
  *out = s.release();
  return RS_OK;
}

int rs_session_feed(rs_session* s, int idx, const uint8_t* shard) {
  DeviceGuard dg;
  if (!s || !shard) return RS_E_ARG;
  std::lock_guard<std::mutex> g(s->mu);
  if (const int rc = s->book.may_feed(idx)) return rc;
  HIPCHK(hipSetDevice(s->device));
  const unsigned flags = s->book.feeds == 0 ? RS_DECODE_IDX_STORE : 0u;  // the first feed stores
  const FeedRoute route = feed_route(s->S, s->inplace_max, s->ctx->pinned.contains(shard, s->S));
  rs_session::Source& src = s->ring[s->next];
  // the slot's last launch has read its shard
  if (src.busy) {
    HIPCHK(hipEventSynchronize(src.done));
    src.busy = false;
  }
  const uint8_t* from = shard;
  uint64_t copies = 0;
  int rc;
  if (route == FeedRoute::kInPlace) {
    if ((rc = src.coherent.ensure(s->S))) return rc;
    std::memcpy(src.coherent.p, shard, s->S);
    from = static_cast<const uint8_t*>(src.coherent.p);
  } else if (route == FeedRoute::kStaged) {
    if ((rc = src.staging.ensure(s->S))) return rc;
    if ((rc = src.dev.ensure(s->S))) return rc;
    std::memcpy(src.staging.p, shard, s->S);
    HIPCHK(hipMemcpyAsync(src.dev.p, src.staging.p, s->S, hipMemcpyHostToDevice, s->stream));
    from = static_cast<const uint8_t*>(src.dev.p);
    copies = 1;
  }
  if ((rc = rs_feed_launch(s->feed, idx, from, flags, s->stream))) return rc;
  HIPCHK(hipEventRecord(src.done, s->stream));
  if (route == FeedRoute::kDirect) {
    // the kernel reads the caller's buffer: the call returns once it has
    HIPCHK(hipEventSynchronize(src.done));
  } else {
    src.busy = true;
    s->next = (s->next + 1) % s->depth;
  }
  s->book.note_feed(idx);
  count(s->ctx, 1, copies);
  return RS_OK;
}

int rs_session_peek(rs_session* s, int idx, uint8_t* out, size_t len) {
  DeviceGuard dg;
  if (!s || !out) return RS_E_ARG;
  std::lock_guard<std::mutex> g(s->mu);
  if (!s->book.has_row(idx) || len > s->S) return RS_E_ARG;
  HIPCHK(hipSetDevice(s->device));
  if (len) HIPCHK(hipMemcpyAsync(out, s->row(idx), len, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  count(s->ctx, 0, len ? 1 : 0);
  return RS_OK;
}

int rs_session_finish(rs_session* s, uint8_t* const* dst, const size_t* dst_lens, uint8_t* const* fix,
                      uint64_t* counts) {
  DeviceGuard dg;
  if (!s) return RS_E_ARG;
  std::lock_guard<std::mutex> g(s->mu);
  const size_t n = static_cast<size_t>(s->k + s->m);
  const size_t nwant = s->rows.size() - s->ncmp;
  if (!dst && nwant) return RS_E_ARG;
  if (const int rc = s->book.may_finish()) return rc;
  const std::vector<int> delivered = s->book.delivered_compared();
  for (size_t i = 0; i < n; ++i) {
    if (dst_lens && s->book.want[i] && dst[i] && dst_lens[i] > s->S) return RS_E_ARG;
    // a fix row belongs to an expected shard or to a compared shard that arrived
    if (fix && fix[i] && !(s->repair && (s->book.expect[i] || (s->book.compare[i] && s->book.fed[i]))))
      return RS_E_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  if (counts) std::fill(counts, counts + n + 1, uint64_t{0});
  int rc, corrupt = 0;
  uint64_t launches = 0, copies = 0;
  int result = RS_OK;
  if (!delivered.empty()) {
    // device fix rows, zeroed, for the indices whose buffer the caller gave
    std::vector<uint8_t*> fixrow(n, nullptr);
    DevBuf fixbuf;
    size_t nfix = 0;
    for (size_t i = 0; fix && i < n; ++i) nfix += fix[i] != nullptr;
    if (nfix) {
      if ((rc = fixbuf.ensure(nfix * s->pitch))) return rc;
      HIPCHK(hipMemsetAsync(fixbuf.p, 0, nfix * s->pitch, s->stream));
      ++copies;
      size_t at = 0;
      for (size_t i = 0; i < n; ++i)
        if (fix[i]) fixrow[i] = static_cast<uint8_t*>(fixbuf.p) + at++ * s->pitch;
    }
    std::vector<uint64_t> blame(n + 1, 0);
    if ((rc = run_final(*s, delivered, fixrow, &corrupt, blame.data()))) return rc;
    ++launches;
    copies += s->repair ? 2 : 1;  // the status words, and a repair plan's counts
    if (s->repair) {
      if (counts) std::copy(blame.begin(), blame.end(), counts);
      if (blame[n]) result = RS_E_CORRUPT;  // a column nobody explains
      // the error rows come back only when something mismatched, and only those that hold one
      std::vector<uint8_t> row(s->S);
      for (size_t i = 0; corrupt && i < n; ++i) {
        if (!fixrow[i] || !blame[i]) continue;
        HIPCHK(hipMemcpy(row.data(), fixrow[i], s->S, hipMemcpyDeviceToHost));
        ++copies;
        for (size_t b = 0; b < s->S; ++b) fix[i][b] ^= row[b];
      }
    } else if (corrupt) {
      result = RS_E_CORRUPT;
    }
  }
  // the wanted rows: straight into rs_host_alloc destinations, one span through staging for the rest
  bool staged = false;
  for (size_t r = s->ncmp; r < s->rows.size(); ++r) {
    const size_t i = static_cast<size_t>(s->rows[r]);
    const size_t len = dst_lens ? dst_lens[i] : s->S;
    if (!dst[i] || !len) continue;
    if (s->ctx->pinned.contains(dst[i], len)) {
      HIPCHK(hipMemcpyAsync(dst[i], static_cast<uint8_t*>(s->rowbuf.p) + r * s->pitch, len, hipMemcpyDeviceToHost,
                            s->stream));
      ++copies;
    } else {
      staged = true;
    }
  }
  if (staged) {
    HIPCHK(hipMemcpyAsync(s->out.p, static_cast<uint8_t*>(s->rowbuf.p) + s->ncmp * s->pitch, nwant * s->pitch,
                          hipMemcpyDeviceToHost, s->stream));
    ++copies;
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  for (size_t r = s->ncmp; staged && r < s->rows.size(); ++r) {
    const size_t i = static_cast<size_t>(s->rows[r]);
    const size_t len = dst_lens ? dst_lens[i] : s->S;
    if (!dst[i] || !len || s->ctx->pinned.contains(dst[i], len)) continue;
    std::memcpy(dst[i], static_cast<const uint8_t*>(s->out.p) + (r - s->ncmp) * s->pitch, len);
  }
  s->book.finished = true;
  count(s->ctx, launches, copies);
  return result;
}

void rs_session_close(rs_session* s) {
  DeviceGuard dg;
  delete s;
}

}  // extern "C"
