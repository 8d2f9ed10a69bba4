// Encode sessions of the C ABI (include/callfs_rs.h): the host route over an
// absorb object. A session keeps one object's m parity rows resident on one device from open to
// close; every piece of the body that arrives is one rs_absorb launch on the session's stream,
// from a slot of a small ring of source buffers, and finish only copies the rows out. Built on
// rs_plan.cpp's public calls alone; a session holds no Lane.
#include <mutex>

#include "host_encode_session.hpp"
#include "rs_internal.hpp"

using namespace callfs;

struct rs_encode_session {
  rs_ctx* ctx = nullptr;
  int device = 0;
  int k = 0, m = 0;
  size_t S = 0, pitch = 0, slot = 0;
  size_t inplace_max = 0;
  std::mutex mu;
  EncodeBook book;
  std::vector<EncodePiece> pieces;
  DevBuf rowbuf;  // row j at rowbuf + j * pitch
  HostBuf out;    // the rows on their way to pageable destinations
  rs_absorb* absorb = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t direct_done = nullptr;  // behind the last launch that reads the caller's buffer
  // one source slot: the piece in host-coherent memory the kernel reads in place, or in staging
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

  uint8_t* row(int j) const { return static_cast<uint8_t*>(rowbuf.p) + static_cast<size_t>(j) * pitch; }
  ~rs_encode_session() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (absorb) rs_absorb_destroy(absorb);
    for (Source& s : ring)
      if (s.done) (void)hipEventDestroy(s.done);
    if (direct_done) (void)hipEventDestroy(direct_done);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

void count(rs_ctx* ctx, uint64_t launches, uint64_t copies) {
  ctx->n_calls.fetch_add(1, std::memory_order_relaxed);
  ctx->n_launches.fetch_add(launches, std::memory_order_relaxed);
  ctx->n_copies.fetch_add(copies, std::memory_order_relaxed);
}

}  // namespace

extern "C" {

int rs_encode_session_open(rs_ctx* ctx, int k, int m, size_t len, rs_encode_session** out) {
  DeviceGuard dg;
  if (const int rc = check_profile(k, m)) return rc;
  if (!ctx || !out) return RS_E_ARG;
  *out = nullptr;
  if (len == 0) return RS_E_SHORT_DATA;
  if (m > kAbsorbMaxRows) return RS_E_UNSUPPORTED;
  if (ctx->devs.empty()) return RS_E_HIP;
  auto s = std::make_unique<rs_encode_session>();
  s->ctx = ctx;
  s->device = ctx->devs[device_slot(ctx->rr.fetch_add(1), 0, ctx->devs.size())]->id;
  s->k = k;
  s->m = m;
  s->book.open(k, len);
  s->S = s->book.S;
  s->pitch = round_up(s->S, kPitchAlign);
  s->slot = encode_session_slot(len, encode_session_chunk());
  s->inplace_max = session_inplace_max();
  HIPCHK(hipSetDevice(s->device));
  int rc;
  const size_t rows_bytes = static_cast<size_t>(m) * s->pitch;
  if ((rc = s->rowbuf.ensure(rows_bytes))) return rc;
  HIPCHK(hipMemset(s->rowbuf.p, 0, rows_bytes));
  if ((rc = s->out.ensure(rows_bytes))) return rc;
  HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&s->direct_done, hipEventDisableTiming));
  s->depth = static_cast<size_t>(session_slots());
  for (size_t q = 0; q < s->depth; ++q) HIPCHK(hipEventCreateWithFlags(&s->ring[q].done, hipEventDisableTiming));
  std::vector<uint8_t*> rows(static_cast<size_t>(m));
  for (int j = 0; j < m; ++j) rows[static_cast<size_t>(j)] = s->row(j);
  if ((rc = rs_absorb_create(ctx, s->device, k, m, s->S, rows.data(), &s->absorb))) return rc;
  *out = s.release();
  return RS_OK;
}

int rs_encode_session_feed(rs_encode_session* s, uint64_t off, const uint8_t* bytes, size_t n) {
  DeviceGuard dg;
  if (!s || !bytes) return RS_E_ARG;
  std::lock_guard<std::mutex> g(s->mu);
  if (const int rc = s->book.may_feed(off, n)) return rc;
  HIPCHK(hipSetDevice(s->device));
  encode_pieces(off, n, s->slot, s->pieces);
  uint64_t launches = 0, copies = 0;
  bool direct = false;
  int rc;
  for (const EncodePiece& p : s->pieces) {
    const uint8_t* piece = bytes + (p.off - off);
    const FeedRoute route = feed_route(p.n, s->inplace_max, s->ctx->pinned.contains(piece, p.n));
    const uint8_t* from = piece;
    if (route == FeedRoute::kDirect) {
      if ((rc = rs_absorb_launch(s->absorb, p.off, p.n, from, s->stream))) return rc;
      direct = true;
    } else {
      rs_encode_session::Source& src = s->ring[s->next];
      // the slot's last launch has read its piece
      if (src.busy) {
        HIPCHK(hipEventSynchronize(src.done));
        src.busy = false;
      }
      if (route == FeedRoute::kInPlace) {
        if ((rc = src.coherent.ensure(s->slot))) return rc;
        std::memcpy(src.coherent.p, piece, p.n);
        from = static_cast<const uint8_t*>(src.coherent.p);
      } else {
        if ((rc = src.staging.ensure(s->slot))) return rc;
        if ((rc = src.dev.ensure(s->slot))) return rc;
        std::memcpy(src.staging.p, piece, p.n);
        HIPCHK(hipMemcpyAsync(src.dev.p, src.staging.p, p.n, hipMemcpyHostToDevice, s->stream));
        from = static_cast<const uint8_t*>(src.dev.p);
        ++copies;
      }
      if ((rc = rs_absorb_launch(s->absorb, p.off, p.n, from, s->stream))) return rc;
      HIPCHK(hipEventRecord(src.done, s->stream));
      src.busy = true;
      s->next = (s->next + 1) % s->depth;
    }
    ++launches;
  }
  if (direct) {
    // a kernel reads the caller's buffer: the call returns once the stream is past it
    HIPCHK(hipEventRecord(s->direct_done, s->stream));
    HIPCHK(hipEventSynchronize(s->direct_done));
  }
  s->book.note_feed(off, n);
  count(s->ctx, launches, copies);
  return RS_OK;
}

int rs_encode_session_peek(rs_encode_session* s, int j, uint8_t* out, size_t n) {
  DeviceGuard dg;
  if (!s || !out) return RS_E_ARG;
  std::lock_guard<std::mutex> g(s->mu);
  if (j < 0 || j >= s->m || n > s->S) return RS_E_ARG;
  HIPCHK(hipSetDevice(s->device));
  if (n) HIPCHK(hipMemcpyAsync(out, s->row(j), n, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  count(s->ctx, 0, n ? 1 : 0);
  return RS_OK;
}

int rs_encode_session_finish(rs_encode_session* s, uint8_t* const* parity, size_t* shard_size) {
  DeviceGuard dg;
  if (!s || !parity) return RS_E_ARG;
  std::lock_guard<std::mutex> g(s->mu);
  for (int j = 0; j < s->m; ++j)
    if (!parity[j]) return RS_E_ARG;
  if (!s->book.complete()) return RS_E_SHORT_DATA;
  HIPCHK(hipSetDevice(s->device));
  // straight into rs_host_alloc destinations, one span through staging for the rest
  uint64_t copies = 0;
  bool staged = false;
  for (int j = 0; j < s->m; ++j) {
    if (s->ctx->pinned.contains(parity[j], s->S)) {
      HIPCHK(hipMemcpyAsync(parity[j], s->row(j), s->S, hipMemcpyDeviceToHost, s->stream));
      ++copies;
    } else {
      staged = true;
    }
  }
  if (staged) {
    HIPCHK(hipMemcpyAsync(s->out.p, s->rowbuf.p, static_cast<size_t>(s->m) * s->pitch, hipMemcpyDeviceToHost,
                          s->stream));
    ++copies;
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  for (int j = 0; staged && j < s->m; ++j) {
    if (s->ctx->pinned.contains(parity[j], s->S)) continue;
    std::memcpy(parity[j], static_cast<const uint8_t*>(s->out.p) + static_cast<size_t>(j) * s->pitch, s->S);
  }
  if (shard_size) *shard_size = s->S;
  s->book.finished = true;
  count(s->ctx, 0, copies);
  return RS_OK;
}

void rs_encode_session_close(rs_encode_session* s) {
  DeviceGuard dg;
  delete s;
}

}  // extern "C"
