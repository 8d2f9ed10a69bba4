/*
 * callfs_rs.h — C ABI of the MI355X-native Reed-Solomon erasure-coding path for CallFS.
 *
 * Drop-in boundary for erasure/codec.go: the Go package keeps its API
 * (NewCodec/Encode/Decode, codec.go:15,21,45) and a cgo shim
 * (erasure/codec_rocm.go, //go:build rocm && cgo — see INTEGRATION.md) binds the
 * functions below. All GF(2^8) arithmetic that the reference delegates to
 * github.com/klauspost/reedsolomon v1.13.3 (go.mod:13) runs here as hand-written
 * HIP kernels for gfx950.
 *
 * Conventions
 *  - Every function returns RS_OK (0) or a negative RS_E_* code.
 *  - No pointer passed in is retained after return (cgo pointer rules).
 *  - Host-memory entry points are synchronous (return after the D2H copy lands).
 *  - All entry points are thread-safe; one rs_ctx may be shared by every request
 *    goroutine, like the shared *Codec at erasure/manager.go:60.
 *  - There is no CPU compute fallback: without a usable HIP device rs_init fails
 *    with RS_E_HIP. Profiles with k+m > 256 (upstream switches to Leopard GF(2^16)
 *    in reedsolomon.New, codec.go:26) return RS_E_UNSUPPORTED and the Go shim keeps
 *    the CPU codec for them.
 */
#ifndef CALLFS_RS_H
#define CALLFS_RS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ABI_VERSION 1

/* ---- error codes (mapped to Go errors by the shim) ---- */
#define RS_OK                 0
#define RS_E_INVALID_PROFILE (-1)  /* erasure.ErrInvalidProfile (errors.go:9; codec.go:22-24,46-48) */
#define RS_E_SHORT_DATA      (-2)  /* reedsolomon.ErrShortData from Split (codec.go:31-34) */
#define RS_E_TOO_FEW_SHARDS  (-3)  /* reedsolomon.ErrTooFewShards from Reconstruct (codec.go:55) */
#define RS_E_SHARD_SIZE      (-4)  /* reedsolomon.ErrShardSize */
#define RS_E_NO_DATA         (-5)  /* reedsolomon.ErrShardNoData */
#define RS_E_CORRUPT         (-6)  /* erasure.ErrShardCorrupted (errors.go:8; codec.go:63-65) */
#define RS_E_INSUFFICIENT    (-7)  /* erasure.ErrInsufficientShards (errors.go:7; codec.go:73-75) */
#define RS_E_UNSUPPORTED     (-8)  /* k+m > 256: Leopard GF(2^16) path, not implemented on GPU */
#define RS_E_HIP             (-9)  /* HIP runtime failure / no device */
#define RS_E_ARG             (-10) /* NULL pointer, short buffer, bad count */
#define RS_E_SINGULAR        (-11) /* reedsolomon.ErrSingular (cannot happen for valid profiles) */
#define RS_E_NOMEM           (-12) /* host or device allocation failed */

typedef struct rs_ctx rs_ctx;
typedef struct rs_plan rs_plan;

/* ---- lifetime ---------------------------------------------------------------------
 * Replaces NewCodec (erasure/codec.go:15-17). device_mask: bit d selects HIP device d;
 * 0 selects every visible device. Host-memory calls are spread over the selected
 * devices (one per call, round-robin). */
int  rs_init(rs_ctx** out, unsigned device_mask);
void rs_shutdown(rs_ctx* ctx);
int  rs_device_count(const rs_ctx* ctx);
int  rs_abi_version(void);
const char* rs_strerror(int code);

/* ---- host-side helpers (no device needed) -------------------------------------------
 * rs_shard_size: S = ceil(len/k) as upstream Split computes it (codec.go:31).
 * rs_encode_matrix: E = V . inv(V[0:k]), (k+m) x k row-major (upstream buildMatrix,
 *   reached via reedsolomon.New at codec.go:26).
 * rs_decode_rows: for a presence mask over n = k+m shards, the first k present
 *   indices (valid), the missing indices, and the rows over the valid shards that
 *   produce every missing shard (data rows of inv(E[valid]); parity rows
 *   P[j].inv(E[valid])), as upstream Reconstruct computes them (codec.go:55).
 *   valid_out: k ints; missing_out: n ints; rows_out: n*k bytes (n_missing*k used). */
int rs_shard_size(int k, int m, int64_t len, int64_t* shard_size);
int rs_encode_matrix(int k, int m, uint8_t* out);
int rs_decode_rows(int k, int m, const uint8_t* present, int* valid_out, int* missing_out,
                   int* n_missing, uint8_t* rows_out);

/* ---- Codec-level, host memory (the cgo shim's two calls) ----------------------------
 * rs_codec_encode replaces Codec.Encode (erasure/codec.go:21-41): Split + Encode.
 *   Writes n = k+m shards of S = ceil(len/k) bytes back to back into shards_out
 *   (shard i at offset i*S; needs out_cap >= n*S). *shard_size receives S.
 *   len == 0 -> RS_E_SHORT_DATA (upstream Split).
 * rs_codec_decode replaces Codec.Decode (erasure/codec.go:45-78): Reconstruct + Verify
 *   + join + trim. shards[i] points to a buffer of at least S bytes for every i;
 *   lens[i] is that shard's length, 0 meaning missing (nil in Go). Missing shards are
 *   reconstructed INTO shards[i] and lens[i] is set to S (Decode mutates its shards
 *   argument in Go). out receives original_size bytes.
 *   Error precedence follows codec.go: profile, shard count/size, too few, corrupt,
 *   insufficient. */
int rs_codec_encode(rs_ctx* ctx, int k, int m, const uint8_t* data, size_t len,
                    uint8_t* shards_out, size_t out_cap, size_t* shard_size);
int rs_codec_decode(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                    uint8_t* out, int64_t original_size);

/* ---- pinned host buffers: zero-copy staging -----------------------------------------
 * rs_host_alloc returns `bytes` of page-locked host memory (page-aligned) that the
 * host-memory entry points above and below DMA from and to directly. When every shard
 * buffer of a call (and, for rs_codec_decode, `out`) lies inside such allocations, the
 * call skips the library's CPU copy through its own pinned staging: H2D, kernels and
 * D2H run on the caller's bytes, and the CPU only enqueues. A server reads request
 * bodies and backend shards straight into these buffers. Calls with any
 * other buffer use the copy-pool staging path as before. Free with rs_host_free
 * (RS_E_ARG for a pointer rs_host_alloc did not return or that was already freed).
 * Freed buffers are kept by the context for reuse: fresh buffers are allocated in 2 MiB
 * granules, and a later rs_host_alloc returns the smallest kept buffer that fits without
 * wasting more than a quarter of it, both sides counted in granules (so a 4 KiB body
 * freed by one request serves the next), without page-locking new memory; a server may
 * allocate a body per request (CALLFS_RS_HOST_POOL_BYTES caps the idle bytes kept,
 * default 4 GiB, 0 = keep none; rs_shutdown releases them). No reference equivalent: Go's
 * io.ReadAll allocations (post_file_enhanced.go:127, manager.go:473,530) are what it
 * replaces on a ROCm build. */
int rs_host_alloc(rs_ctx* ctx, size_t bytes, void** out);
int rs_host_free(rs_ctx* ctx, void* p);

/* ---- Encoder-level, host memory (reedsolomon.Encoder methods used by codec.go) -----
 * rs_encode:      enc.Encode(shards)      (codec.go:36)  data: k ptrs, parity: m ptrs, S bytes each
 * rs_reconstruct: enc.Reconstruct(shards) (codec.go:55)  same buffer/lens contract as rs_codec_decode
 * rs_verify:      enc.Verify(shards)      (codec.go:59)  *ok = 1 when parity matches */
int rs_encode(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* const* data,
              uint8_t* const* parity);
int rs_reconstruct(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens);
int rs_verify(rs_ctx* ctx, int k, int m, const uint8_t* const* shards, const size_t* lens,
              int* ok);

/* ---- Batched, host memory (many independent stripes per call) ----------------------
 * Not in the reference API: for callers holding many objects at once (repair of every
 * object that lost one shard, bulk re-encode, a server batching small uploads). A batch
 * whose stripes all share one shard size and one presence mask runs as one uniform
 * pipeline in which small stripes are packed many per H2D / launch / D2H. A batch of
 * different shard sizes or masks runs as one ragged pipeline: the stripes (column parts of
 * the large ones) are packed into chunks of CALLFS_RS_CHUNK_BYTES whatever their sizes and
 * masks, and a chunk costs one H2D, one launch per group of 16 rows and one D2H -- or one
 * dispatch in place on host-coherent staging for batches of at most
 * CALLFS_RS_SMALL_MAX_BYTES, or launches on the caller's own buffers when all of them
 * are rs_host_alloc memory -- so the call's cost follows its bytes, not the number of sizes
 * and masks in it. (Reconstructs with verify == 0 run one such pipeline per missing-shard
 * count.) CALLFS_RS_RAGGED_BATCH=0 (read once per process) runs one pipeline per
 * (S, presence) group instead.
 * rs_encode_batch: stripe b has sizes[b]-byte shards, data[b*k + i] / parity[b*m + j]
 *   (= rs_encode per stripe, codec.go:36). sizes[b] == 0 -> status[b] = RS_E_NO_DATA.
 * rs_reconstruct_batch: shards[b*n + i] / lens[b*n + i] with rs_reconstruct's contract
 *   per stripe (codec.go:55); verify != 0 also re-checks the present parity beyond the
 *   first k (codec.go:59) -> status[b] = RS_E_CORRUPT for that stripe alone.
 * status[b] receives each stripe's code (RS_OK, RS_E_NO_DATA, RS_E_SHARD_SIZE,
 * RS_E_TOO_FEW_SHARDS, RS_E_ARG, RS_E_CORRUPT). Returns RS_OK when every stripe is OK,
 * else the first nonzero status in stripe order; a call-level error (RS_E_ARG,
 * RS_E_INVALID_PROFILE, RS_E_HIP, RS_E_NOMEM) is returned directly with status[]
 * unspecified. */
int rs_encode_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                    const uint8_t* const* data, uint8_t* const* parity, int* status);
int rs_reconstruct_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                         size_t* lens, int verify, int* status);

/* ---- Codec-level batches, host memory (many objects per call) -------------------------
 * Not in the reference API: Codec.Encode / Codec.Decode (codec.go:21-78) for many objects
 * of one profile at once, for a server batching small uploads or downloads. Objects go in
 * and come out: Split (codec.go:31) happens on the way into the pipeline's staging and the
 * join / trim (codec.go:67-77) on the way out of it, so no object is copied a second time,
 * and every object gets the status the single-object call would return for it. The
 * runnable objects run as the stripes of rs_encode_batch / rs_reconstruct_batch do: one
 * uniform pipeline when they share one shard size and one presence mask, else one ragged
 * pipeline (staged, one dispatch in place for at most CALLFS_RS_SMALL_MAX_BYTES, or launches
 * on the caller's buffers when every buffer of every runnable object -- data, shards_out,
 * shards and out -- is rs_host_alloc memory); CALLFS_RS_RAGGED_BATCH=0 runs one pipeline
 * per (S, presence) group.
 * rs_codec_encode_batch: object b is handled as rs_codec_encode(ctx, k, m, data[b],
 *   lens[b], shards_out[b], out_caps[b], &shard_sizes[b]) handles it: n = k+m shards of
 *   S_b = ceil(lens[b]/k) bytes back to back in shards_out[b], bytes [lens[b], k*S_b) zero.
 *   status[b]: RS_OK; RS_E_SHORT_DATA for lens[b] == 0; RS_E_ARG for a NULL data[b] or
 *   shards_out[b] or out_caps[b] < n*S_b (shard_sizes[b] is written for RS_OK alone).
 *   shards_out[b] == data[b] (the object split in place) is allowed, and buffers of ONE
 *   object that overlap partly are handled as rs_codec_encode handles them; buffers of
 *   different objects must not overlap. No byte at or beyond shards_out[b] + n*S_b is
 *   written.
 * rs_codec_decode_batch: object b has shards[b*n + i] / lens[b*n + i] with
 *   rs_codec_decode's contract (0 = missing; missing shards are rebuilt into their buffers
 *   and their lens set to S when status[b] is RS_OK, RS_E_CORRUPT or RS_E_INSUFFICIENT, as
 *   upstream Reconstruct has run by then); out[b] receives original_sizes[b] bytes. An
 *   object with every shard present is still verified and joined. status[b], in this
 *   order: RS_E_NO_DATA / RS_E_SHARD_SIZE (shard count / size checks), RS_E_TOO_FEW_SHARDS,
 *   RS_E_ARG (a NULL shard buffer, a negative size, a NULL out[b] with a positive size),
 *   RS_E_CORRUPT (Verify fails, for that object alone), RS_E_INSUFFICIENT
 *   (k*S < original_sizes[b]). out[b] is unspecified unless status[b] is RS_OK and is never
 *   written at or beyond original_sizes[b].
 * Both: the profile errors (RS_E_INVALID_PROFILE, RS_E_UNSUPPORTED), a NULL array and
 * batch < 0 (RS_E_ARG) are call-level, checked first, and leave status[] unspecified, as do
 * RS_E_HIP / RS_E_NOMEM; batch == 0 returns RS_OK. Otherwise the call returns RS_OK or the
 * first nonzero status in object order. */
int rs_codec_encode_batch(rs_ctx* ctx, int k, int m, int batch,
                          const uint8_t* const* data, const size_t* lens,
                          uint8_t* const* shards_out, const size_t* out_caps,
                          size_t* shard_sizes, int* status);
int rs_codec_decode_batch(rs_ctx* ctx, int k, int m, int batch,
                          uint8_t* const* shards, size_t* lens,
                          uint8_t* const* out, const int64_t* original_sizes, int* status);

/* ---- Checksummed codec batches -----------------------------------
 * The batches above with ShardChecksum (SHA-256, codec.go:81-84) of every shard taken on
 * the way through the pipeline: what Manager.StoreFile computes beside Codec.Encode
 * (manager.go:185) and what Manager.RetrieveFile checks before Codec.Decode
 * (manager.go:283-296). They take the ragged pipeline's staged transport whatever the
 * batch holds. A shard that passes through a chunk whole is hashed in the chunk's device
 * mirror or by the library's copy threads (CALLFS_RS_SUMS_DEVICE = auto / 0 / 1); a shard
 * cut over several chunks is hashed by the copy threads. Both give the same bytes.
 * rs_codec_encode_batch_sums: rs_codec_encode_batch (same bytes in shards_out, same
 *   shard_sizes, statuses, precedence and overlap rules), and digests[(b*n + i)*32 ..] holds
 *   the SHA-256 of shard i of object b over all S_b bytes, the zero pad included. digests
 *   has batch*n*32 bytes; entries are written for objects of status RS_OK alone.
 * rs_codec_decode_batch_sums: expected has batch*n*32 bytes (entries of missing shards are
 *   ignored), bad batch*n bytes. Admission is rs_codec_decode_batch's on the shards as given
 *   (a present shard of the wrong length is RS_E_SHARD_SIZE, where the manager would see a
 *   checksum mismatch: drop such a shard before the call). For an admitted object every
 *   entry of bad is written: 1 for a present shard whose SHA-256 differs from its expected
 *   digest, else 0; it is 0 for objects refused at admission. A bad shard counts as missing:
 *   from there the object's outcome, status and precedence are rs_codec_decode_batch's with
 *   that shard's length zero (it is rebuilt into its own buffer, Verify runs over what is
 *   left, out[b] is joined and trimmed). With fewer than k good shards left status[b] is
 *   RS_E_TOO_FEW_SHARDS and the object's buffers and lens are left as given. Rebuilt shards
 *   are not checked against their expected digests.
 * Both: call-level errors and batch == 0 as above; digests, expected and bad are arrays
 * like the others (NULL with batch > 0: RS_E_ARG). rs_host_counters: `launches` also counts
 * one per chunk hashed on the device; a call without a mismatch enqueues the copies of the
 * plain call on the same transport, and the objects with a mismatch run a second time. */
int rs_codec_encode_batch_sums(rs_ctx* ctx, int k, int m, int batch,
                               const uint8_t* const* data, const size_t* lens,
                               uint8_t* const* shards_out, const size_t* out_caps,
                               size_t* shard_sizes, uint8_t* digests, int* status);
int rs_codec_decode_batch_sums(rs_ctx* ctx, int k, int m, int batch,
                               uint8_t* const* shards, size_t* lens, const uint8_t* expected,
                               uint8_t* const* out, const int64_t* original_sizes,
                               uint8_t* bad, int* status);

/* ---- Only the shards a caller asks for --------------------------
 * Upstream ReconstructSome(shards, required) and ReconstructData for host memory. A download
 * keeps the joined data alone and a repair wants the one shard its node lost: these calls
 * rebuild nothing else. required holds k+m flags per stripe (batch*(k+m) for the batch call;
 * nonzero = wanted), or NULL: every missing shard is wanted, and the call is then exactly
 * rs_reconstruct / rs_reconstruct_batch (same work, same rs_host_counters).
 *   - A missing shard whose flag is set is rebuilt, bit-exact with rs_reconstruct, and its
 *     lens entry becomes S.
 *   - A missing shard whose flag is clear is neither written nor read: its pointer may be
 *     NULL and its lens entry stays 0.
 *   - Flags on present shards are ignored. With verify != 0 the present shards beyond the
 *     first k are compared as in rs_reconstruct_batch (RS_E_CORRUPT per stripe).
 * Contract and status values are rs_reconstruct's / rs_reconstruct_batch's. A stripe that
 * wants nothing (and, with verify, has nothing to compare) is RS_OK without device work; a
 * call of such stripes alone reaches no device and moves no counter.
 * rs_codec_decode_data / rs_codec_decode_data_batch are rs_codec_decode / _batch with the
 * data shards wanted (ReconstructData in Reconstruct's place): `out`, the joins, trims,
 * error precedence and RS_E_CORRUPT from the compared shards are the same, missing parity
 * shards stay missing (lens 0) and their buffers may be NULL. */
int rs_reconstruct_some(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                        const uint8_t* required);
int rs_reconstruct_some_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                              size_t* lens, const uint8_t* required, int verify, int* status);
int rs_codec_decode_data(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                         uint8_t* out, int64_t original_size);
int rs_codec_decode_data_batch(rs_ctx* ctx, int k, int m, int batch,
                               uint8_t* const* shards, size_t* lens,
                               uint8_t* const* out, const int64_t* original_sizes, int* status);

/* ---- Parity updated in place, host memory -------------------------
 * Upstream Update(shards, newDatashards) and EncodeIdx(dataShard, idx, parity): the parity is
 * read, changed and written back; no unchanged data shard is read, and data shards are never
 * written ("the data shards will remain the same").
 * rs_update: new_data[i] == NULL means data shard i is unchanged; for every other i,
 *   parity[j] ^= P[j][i] * (old_data[i] ^ new_data[i]) over S bytes, after which the parity is
 *   what rs_encode of the new data gives. A changed shard whose old_data entry is NULL is
 *   RS_E_ARG (upstream ErrInvalidInput), S == 0 with a change RS_E_NO_DATA. Nothing changed:
 *   RS_OK with no device work and no counter moved.
 * rs_encode_idx: parity[j] ^= P[j][idx] * shard, added to whatever the parity holds
 *   (upstream has the caller zero it before the first shard); the k shards of a stripe may
 *   arrive in any order. idx outside [0, k) is RS_E_ARG (upstream ErrInvalidShardIdx).
 * rs_update_batch: stripe b has sizes[b]-byte shards, old_data / new_data[b*k + i] and
 *   parity[b*m + j], each stripe as rs_update; old_data == NULL (the array) is EncodeIdx mode
 *   for the whole batch (every non-NULL new_data entry is added). status[b] is RS_OK,
 *   RS_E_NO_DATA or RS_E_ARG (a changed shard without old bytes, a NULL parity pointer); the
 *   return value follows rs_encode_batch's rule. No parity byte of one stripe may overlap a
 *   parity byte of another stripe or any source.
 * rs_codec_overwrite: `shards` are the n = k+m S-byte shards of an object laid out as
 *   rs_codec_encode lays it (object byte x in data shard x / S at column x % S). Bytes
 *   [offset, offset + len) of the object become `data`: the affected parity columns are
 *   updated through one rs_update_batch of at most three stripes (disjoint column intervals,
 *   each with its own changed shards), then `data` is copied into the data shards. Afterwards
 *   the shards equal rs_codec_encode of the overwritten object bit for bit, and no column
 *   outside the range is touched in any shard. Every data shard the range touches and all m
 *   parity shards must be non-NULL (RS_E_ARG), as must data; a range past k*S, offset < 0 or
 *   len == 0 is RS_E_ARG. `data` must not overlap the shards.
 * All four take the staged ragged pipeline (a chunk: one H2D of the changed sources and the
 * parity rows, one launch per group of 16 parity rows, one D2H of the parity rows), whatever
 * memory the buffers are in, on one device; rs_host_counters counts them like the other calls. */
int rs_update(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* const* old_data,
              const uint8_t* const* new_data, uint8_t* const* parity);
int rs_encode_idx(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* shard, int idx,
                  uint8_t* const* parity);
int rs_update_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                    const uint8_t* const* old_data, const uint8_t* const* new_data,
                    uint8_t* const* parity, int* status);
int rs_codec_overwrite(rs_ctx* ctx, int k, int m, size_t S, uint8_t* const* shards,
                       int64_t offset, const uint8_t* data, size_t len);

/* ---- Progressive decode, host memory -------------------------------
 * Upstream DecodeIdx(dst, expectInput, input) for stripes in host memory: expect, input, dst and
 * flags exactly as for rs_plan_create_decode_idx (below), over n = k+m entries per stripe, and
 * the same result: merge adds the delivered shards' terms into the wanted shards, store
 * (RS_DECODE_IDX_STORE) stores them without reading the wanted shards. After every expected shard
 * has been delivered once, in any order and any grouping of calls, dst holds bit for bit what
 * rs_reconstruct gives with exactly those k shards present -- from zeroed destinations, or when
 * the first call stores.
 * rs_decode_idx: one stripe of S-byte shards. Errors in the plan constructor's order: the
 *   profile; a NULL ctx, dst, expect or input, or a flag bit other than RS_DECODE_IDX_STORE
 *   (RS_E_ARG); the expect count (RS_E_TOO_FEW_SHARDS below k, RS_E_ARG above); a misplaced
 *   pointer (RS_E_ARG); S == 0 with both an input and a dst (RS_E_NO_DATA).
 * rs_decode_idx_batch: stripe b has sizes[b]-byte shards and entries b*n + i of dst, expect and
 *   input. The profile, NULL arrays, batch < 0 and the flag bits fail the call; the per-stripe
 *   refusals land in status[b] (in the same order) and the other stripes run. The return value
 *   follows rs_update_batch's rule. No dst byte of one stripe may overlap a dst byte of another
 *   stripe or any input.
 * A stripe with no input or no wanted shard keeps every byte; a call in which no stripe has both
 * reaches no device, moves no counter and returns RS_OK.
 * Both take the staged ragged pipeline on one device, whatever memory the buffers are in. A
 * chunk: one H2D of metadata and the delivered shards; in merge mode a second H2D of the wanted
 * shards' current bytes -- A STORE CALL DOES NOT UPLOAD THE WANTED SHARDS, and `copies` of
 * rs_host_counters shows it (2 per store chunk, 3 per merge chunk); one launch per group of 16
 * wanted rows; one D2H of the wanted rows. A stripe above CALLFS_RS_CHUNK_BYTES is cut into column
 * parts. Every call pays its own round trip: the accumulators do not stay on the device between
 * calls (use a decode-idx plan for that). rs_host_counters counts the calls like the others. */
#define RS_DECODE_IDX_STORE 1u
int rs_decode_idx(rs_ctx* ctx, int k, int m, size_t S, uint8_t* const* dst,
                  const uint8_t* expect, const uint8_t* const* input, unsigned flags);
int rs_decode_idx_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                        uint8_t* const* dst, const uint8_t* expect,
                        const uint8_t* const* input, unsigned flags, int* status);

/* ---- Progressive Verify, host memory --------------------------------
 * rs_decode_idx and rs_decode_idx_batch with compared shards: expect, input, dst, check and flags
 * exactly as for rs_plan_create_decode_check (below), the accumulators in host memory, and the
 * same result. With RS_DECODE_CHECK_FINAL a stripe in which some compared shard differs from what
 * the expected shards imply is RS_E_CORRUPT -- rs_decode_check's return value, status[b] of a
 * batch -- and its wanted shards are delivered all the same, as upstream Decode delivers them
 * before Verify fails; no check row is written.
 * rs_decode_check: one stripe of S-byte shards. Errors in the plan constructor's order.
 * rs_decode_check_batch: as rs_decode_idx_batch; the profile, NULL arrays (check included),
 *   batch < 0 and an unknown flag bit fail the call, the per-stripe refusals land in status[b].
 * A stripe that is in no launch -- no input, or no wanted and no check row; under FINAL a check
 * row alone puts it into the launch -- keeps every byte; a call in which no stripe is reaches no
 * device, moves no counter and returns RS_OK.
 * Both take rs_decode_idx's staged pipeline, with the check rows staged as output rows: a chunk
 * is one H2D of metadata and the delivered shards (final: and the chunk's zeroed status words);
 * in merge mode a second H2D of the wanted and check rows' current bytes; one launch per group of
 * 16 rows; one D2H of the rows, which under FINAL starts at the status words, is of them alone
 * when the call has no wanted row, and from which no check row is copied back. `copies` of
 * rs_host_counters: 2 per store chunk, 3 per merge chunk, final or not. A stripe above
 * CALLFS_RS_CHUNK_BYTES is cut into column parts, and its flag is the OR of its parts' flags. The
 * accumulators do not stay on the device between calls (use a decode-check plan for that). */
int rs_decode_check(rs_ctx* ctx, int k, int m, size_t S, uint8_t* const* dst, uint8_t* const* check,
                    const uint8_t* expect, const uint8_t* const* input, unsigned flags);
int rs_decode_check_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                          uint8_t* const* dst, uint8_t* const* check, const uint8_t* expect,
                          const uint8_t* const* input, unsigned flags, int* status);

/* ---- Progressive repair, host memory --------------------------------
 * The final rs_decode_check call that repairs what it flags: expect, input, dst, check, fix and
 * flags (0 or RS_DECODE_IDX_STORE; the call is always final) exactly as for
 * rs_plan_create_decode_repair (below), every buffer in host memory, and the same result: the
 * wanted shards with the error of every explained column taken out, and the error values XORed
 * into the fix buffers the caller gave (XOR in place: a zeroed buffer ends as the error row, the
 * shard as delivered ends restored; fix[i] may be input[i]).
 * counts: batch * (k+m+1) words, zeroed and filled by the call, NULL allowed: entry i of stripe b
 *   is the number of byte columns blamed on shard i, entry k+m the number left unexplained.
 * status[b] (rs_decode_repair's return value): RS_OK for a clean stripe and for a stripe whose
 *   mismatching columns were all explained -- its counts say what was repaired; RS_E_CORRUPT when
 *   a column is unexplained (always, with fewer than three compared shards), the wanted shards
 *   delivered all the same as upstream Decode delivers them; the stripe's own refusal in the plan
 *   constructor's order otherwise (the expect count; a misplaced pointer, fix included; more than
 *   16 rows: RS_E_UNSUPPORTED; a zero size in the launch), the other stripes running.
 * rs_decode_repair_batch: the profile, NULL arrays (fix included; counts may be NULL), batch < 0
 *   and an unknown flag bit fail the call. A call in which no stripe is in the launch reaches no
 *   device, moves no counter and returns RS_OK.
 * Both are a run of rs_decode_check's staged pipeline. A chunk is a final decode-check chunk;
 * the fix pointer table goes up in a copy of its own; the counts and the fix rows (one per
 * expected and compared shard of an item) live in the chunk's device mirror alone, zeroed there:
 * no fix row is uploaded. The status words and wanted rows come back in one D2H, the counts in a
 * second, and then only the fix rows with a nonzero count whose buffer the caller gave, one copy
 * each, XORed into the caller's buffer. `copies` of rs_host_counters: 4 per store chunk, 5 per
 * merge chunk, plus one per fix row that came back. A stripe above CALLFS_RS_CHUNK_BYTES is cut
 * into column parts: counts add and flags OR. The staged transport alone. */
int rs_decode_repair(rs_ctx* ctx, int k, int m, size_t S, uint8_t* const* dst, uint8_t* const* check,
                     uint8_t* const* fix, const uint8_t* expect, const uint8_t* const* input,
                     unsigned flags, uint64_t* counts);
int rs_decode_repair_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                           uint8_t* const* dst, uint8_t* const* check, uint8_t* const* fix,
                           const uint8_t* expect, const uint8_t* const* input, unsigned flags,
                           int* status, uint64_t* counts);

/* ---- counters of the host-memory path -----------------------------------------------
 * Monotonic per-context counts (relaxed atomics; what an operator graphs, and what shows
 * that a batch cost one round trip):
 *   calls         host-memory entry-point calls that reached a device
 *   chunks        chunks sent
 *   launches      compute launches, one per launch group per chunk (slices of one group
 *                 count once)
 *   copies        H2D / D2H / memset dispatches enqueued for host-memory calls (table
 *                 uploads included)
 *   ragged_calls  batch calls that took the ragged path */
typedef struct rs_host_counters {
  uint64_t calls;
  uint64_t chunks;
  uint64_t launches;
  uint64_t copies;
  uint64_t ragged_calls;
} rs_host_counters;
int rs_host_counters_read(const rs_ctx* ctx, rs_host_counters* out);

/* ---- device-resident plans (batched stripes, graph-capturable launches) -------------
 * A plan fixes (k, m, S, batch, presence mask) and the device pointers of every
 * stripe's n shards: shards[b*n + i] is shard i of stripe b (device memory, S bytes).
 * present == NULL means "encode" (data present, parity missing). Launching a plan
 * computes every missing shard of every stripe from the first k present ones and
 * re-checks the remaining present parity (the Verify of codec.go:59), OR-ing 1 into
 * the plan's device status word on mismatch. rs_plan_launch only enqueues work on
 * `stream` (a hipStream_t; NULL = the null stream) — no allocation, no sync.
 * rs_plan_status synchronises `stream`, sets *corrupt when any stripe's verify rows
 * mismatched since the last status call, and clears the flags;
 * rs_plan_stripe_status does the same per stripe (flags: `batch` ints, nonzero =
 * that object is corrupt — ErrShardCorrupted for it alone). rs_plan_bytes: algorithmic
 * HBM bytes one launch moves (reads of the k+verify inputs + writes of the missing
 * shards). */
int  rs_plan_create(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                    const uint8_t* present, uint8_t* const* shards, rs_plan** out);
int  rs_plan_launch(rs_plan* plan, void* stream);
int  rs_plan_status(rs_plan* plan, void* stream, int* corrupt);
int  rs_plan_stripe_status(rs_plan* plan, void* stream, int* flags);
/* rs_plan_launch that also times its kernels (measurement; no upstream counterpart):
 * start_event / stop_event (hipEvent_t, created by the caller, either may be NULL) are
 * recorded by the launch's first kernel dispatch when it starts and by its last when it
 * ends (hipExtLaunchKernel), so hipEventElapsedTime gives the kernels' own time, without
 * the stream's gap before the first and after the last (what rocprofv3's kernel trace
 * reports). */
int  rs_plan_launch_timed(rs_plan* plan, void* stream, void* start_event, void* stop_event);
uint64_t rs_plan_bytes(const rs_plan* plan);
void rs_plan_destroy(rs_plan* plan);

/* Tile-order tuning (no upstream counterpart; an autotuner for repeated launches).
 * Which order of column tiles HBM serves best for a shape varies between MI355X boxes
 * by 1-2 %. rs_plan_tune warms the device up in the rule's order (~150 ms
 * of launches), then times each launch group of the plan in every
 * tile order its kernel offers (`reps` launches per order, three rounds) and keeps the
 * fastest for later rs_plan_launch calls; the measured rule's order stays unless another
 * is > 1 % faster. Synchronous on `stream`; RS_E_ARG while `stream` is capturing. The
 * tuning launches recompute the plan's outputs from its inputs (same bytes; Verify rows
 * may flag status exactly as rs_plan_launch would). orders (NULL when max_groups == 0):
 * the chosen order per launch group, up to max_groups entries (RS_ORDER_* or -1 = the
 * launch has no choice). */
#define RS_ORDER_CONSECUTIVE 0
#define RS_ORDER_GROUP8 1
#define RS_ORDER_GROUP2 2
#define RS_ORDER_SEG8 3
#define RS_ORDER_SEG16 4
/* consecutive tiles, J = 8 / 32 of them per XCD in turn */
#define RS_ORDER_XCD8 5
#define RS_ORDER_XCD32 6
/* misaligned shards (upstream Split layout at odd S): the kernel that realigns loads and
 * parity stores in registers, RS_ORDER_REALIGN + the tile order it runs in (consecutive,
 * XCD8 or XCD32); on such launches RS_ORDER_0..6 name the plain kernel with unaligned
 * 16-B accesses in that tile order */
#define RS_ORDER_REALIGN 32
/* the launch group's bit-sliced kernel: an XOR network over bit planes
 * generated for the group's coefficient block and compiled at plan time (hiprtc; cached on
 * disk; past 2,048 coefficients per plan the blocks compile in the background while the plan
 * runs the nibble-table kernels), RS_ORDER_BITSLICE + the tile order it runs in (RS_ORDER_0..6);
 * pinning one waits for its compile */
#define RS_ORDER_BITSLICE 256
int  rs_plan_tune(rs_plan* plan, void* stream, int reps, int* orders, int max_groups);
/* Sets the tile order of launch groups 0..n-1 (the others: the rule) to orders[i], as
 * rs_plan_tune would: RS_ORDER_* that the group's kernel has an instance of (what
 * rs_plan_tune times, and XCD8 / XCD32 on aligned shards), or -1 for the rule. RS_E_ARG if any entry is not offered or n
 * exceeds rs_plan_groups; the plan is then unchanged. For orders tuned once and kept. */
int  rs_plan_set_orders(rs_plan* plan, const int* orders, int n);
/* The kernel form each launch group of the next rs_plan_launch runs, up to max_groups
 * entries: the pinned or tuned order, else the rule's (RS_ORDER_BITSLICE + its tile order
 * where the rule gives the group the bit-sliced kernel; the codes rs_plan_tune reports).
 * Returns the number of launch groups, or RS_E_ARG. */
int  rs_plan_forms(const rs_plan* plan, int* forms, int max_groups);
/* The tune table: every rs_plan_tune records its choice per launch shape
 * (device, k, rows, tiles-per-stripe bucket, address alignment, written / compared rows,
 * misalignment), and launches with no order of their own -- untuned plans, the host-memory
 * calls -- take the recorded form for their shape before the built-in rule. With
 * CALLFS_RS_TUNE_TABLE=<file> the table is read from and written back to that file, so a
 * box is tuned once. rs_tune_table_reset forgets every entry and binds the table to `path`
 * (NULL: CALLFS_RS_TUNE_TABLE, or memory only); rs_tune_table_entries counts them. */
int  rs_tune_table_reset(const char* path);
int  rs_tune_table_entries(void);
/* Measurement only (no upstream counterpart): enqueues the plan's launch groups as a
 * traffic ceiling of the same shape, on the production grid, tile order and slicing, for
 * a roofline denominator measured in the same process (bench.py):
 *   RS_CEIL_READ      the plan's read streams alone (k inputs + compared rows);
 *   RS_CEIL_WRITE     its write streams alone (leaves junk in the written shards:
 *                     relaunch the plan before relying on them).
 * Any other mode returns RS_E_ARG. (The development tools' A/B build, built on demand with
 * `python callfs_amd/build.py --ab`, adds the kernel's no-lookup form and aligned-window
 * probes: tools/callfs_rs_ab.h.) */
#define RS_CEIL_READ 1
#define RS_CEIL_WRITE 2
int  rs_plan_launch_ceiling(rs_plan* plan, void* stream, int mode);
/* The same, with its kernels timed as rs_plan_launch_timed times the plan's. */
int  rs_plan_launch_ceiling_timed(rs_plan* plan, void* stream, int mode, void* start_event,
                                  void* stop_event);
/* Launch groups of a plan (the `orders` entries rs_plan_tune can fill): one per up to 16
 * written or compared rows; 0 for a NULL plan. */
int  rs_plan_groups(const rs_plan* plan);

/* One-shot device-resident calls (build + launch + free; tables cached per profile).
 * Same pointer layout as rs_plan_create; synchronous on `stream`. rs_decode_dev
 * returns RS_E_CORRUPT when the verify rows mismatch. */
int rs_encode_dev(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                  uint8_t* const* shards, void* stream);
int rs_decode_dev(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                  const uint8_t* present, uint8_t* const* shards, void* stream);

/* ---- mixed plans: every stripe its own presence mask ----------
 * present holds batch*(k+m) flags, stripe b's mask at present + b*(k+m) (nonzero =
 * present); shards as for rs_plan_create. One launch per launch group reconstructs and
 * verifies the whole batch: each stripe's missing shards are computed from its own first
 * k present shards and its remaining present shards are compared, bit-exact with a
 * uniform plan of that stripe's mask. Any stripe with fewer than k present shards fails
 * the call with RS_E_TOO_FEW_SHARDS and creates nothing (filter such stripes out first).
 * When every stripe has the same mask the call builds exactly what rs_plan_create builds
 * (same kernel forms, bit-sliced ones included). Otherwise the plan runs the mixed
 * nibble-table kernels: no bit-sliced kernel, no hiprtc compile, no tune-table entry, one
 * tile order. The returned plan works with rs_plan_launch, _launch_timed, _status,
 * _stripe_status, _bytes, _groups, _forms and _destroy as any plan does (launches only
 * enqueue: no allocation, no sync; graph-capturable). For a mixed plan
 *   rs_plan_bytes   returns batch*(k+m)*S (every shard of every stripe is read, compared or written);
 *   rs_plan_forms   reports RS_ORDER_MIXED + the tile order (RS_ORDER_CONSECUTIVE);
 *   rs_plan_tune    returns RS_OK, times nothing and fills orders with -1;
 *   rs_plan_set_orders accepts only -1 entries (RS_E_ARG for anything else);
 *   rs_plan_launch_ceiling / _ceiling_timed return RS_E_ARG.
 * rs_decode_dev_mixed is the one-shot form (build + launch + status + free; synchronous on
 * `stream`); it returns RS_E_CORRUPT when any stripe's compared shards mismatch. */
#define RS_ORDER_MIXED 512
int rs_plan_create_mixed(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                         const uint8_t* present, uint8_t* const* shards, rs_plan** out);
int rs_decode_dev_mixed(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                        const uint8_t* present, uint8_t* const* shards, void* stream);

/* ---- ragged plans: every stripe its own shard size as well ------
 * Objects have their own lengths, so a repair, scrub or re-encode batch has as many shard
 * sizes as objects. sizes holds `batch` shard sizes: every shard of stripe b is sizes[b]
 * bytes. present holds batch*(k+m) flags as for rs_plan_create_mixed, or NULL: every stripe
 * is then an encode (data present, parity missing). shards as for rs_plan_create.
 * Stripe b is computed exactly as a mixed plan of shard size sizes[b] with the mask
 * present + b*(k+m) would compute it: its missing shards are written from its first k
 * present shards, its remaining present shards are compared, and the corruption flags are
 * per stripe. No byte at or beyond sizes[b] of any shard of stripe b is read or written
 * (shards may touch each other; misaligned shards take unaligned 16-B accesses).
 * Errors, each of which creates nothing: RS_E_ARG for batch < 1 or a NULL sizes / shards /
 * out; RS_E_NO_DATA when any sizes[b] is 0; RS_E_TOO_FEW_SHARDS when any stripe has fewer
 * than k present shards; the profile errors of rs_plan_create_mixed.
 * When all sizes are equal the call returns exactly what rs_plan_create_mixed returns for
 * that S (the uniform plan when the masks are equal too; same kernel forms, bit-sliced ones
 * included). Otherwise the plan is a ragged plan: one launch per launch group over a tile
 * map of the whole batch, no bit-sliced kernel, no hiprtc compile, no tune-table entry, one
 * tile order. It works with rs_plan_launch, _launch_timed (which only enqueue: no
 * allocation, no sync; graph-capturable), _status, _stripe_status, _groups and _destroy as
 * any plan does. For a ragged plan
 *   rs_plan_bytes   returns (k+m) * the sum of sizes[b];
 *   rs_plan_forms   reports RS_ORDER_RAGGED + RS_ORDER_CONSECUTIVE;
 *   rs_plan_tune    returns RS_OK, times nothing and fills orders with -1;
 *   rs_plan_set_orders accepts only -1 entries (RS_E_ARG for anything else);
 *   rs_plan_launch_ceiling / _ceiling_timed return RS_E_ARG.
 * rs_decode_dev_ragged is the one-shot form (build + launch + status + free; synchronous on
 * `stream`); it returns RS_E_CORRUPT when any stripe's compared shards mismatch. */
#define RS_ORDER_RAGGED 1024
int rs_plan_create_ragged(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                          const uint8_t* present, uint8_t* const* shards, rs_plan** out);
int rs_decode_dev_ragged(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                         const uint8_t* present, uint8_t* const* shards, void* stream);

/* ---- required plans: only the missing shards a caller wants ------
 * Upstream ReconstructSome(shards, required) / ReconstructData for device-resident batches:
 * a download needs its data shards alone, a repair the one shard its node lost. sizes,
 * present and shards as for rs_plan_create_ragged; required holds batch*(k+m) flags beside
 * present's (nonzero = wanted), or NULL: every missing shard is wanted.
 *   - A missing shard whose flag is set is rebuilt, bit-exact with rs_plan_create_ragged.
 *   - A missing shard whose flag is clear is neither written nor read: its pointer is never
 *     passed to a kernel and may be NULL.
 *   - Flags on present shards are ignored; present shards beyond the first k are compared
 *     as in every plan, and the corruption flags are per stripe.
 * Errors are those of rs_plan_create_ragged. Routing, in this order:
 *   1. required == NULL, present == NULL or every missing shard wanted: exactly what
 *      rs_plan_create_ragged returns.
 *   2. all sizes equal and every stripe the same mask and wanted set: the uniform plan of
 *      rs_plan_create over the wanted rows alone (every kernel form, tile orders, tuning and
 *      ceilings as for any uniform plan). When no row is left (exactly k shards present,
 *      nothing wanted) the plan has 0 launch groups, its launch enqueues nothing and
 *      rs_plan_bytes is 0.
 *   3. otherwise a required plan: a ragged plan whose stripes have their own row counts,
 *      each launch group over a tile map of the stripes that have a row in it. Stripe b
 *      with w_b wanted missing shards and c_b compared ones costs r_b = w_b + c_b rows; a
 *      stripe with r_b = 0 is in no launch. It works with rs_plan_launch, _launch_timed
 *      (which only enqueue: no allocation, no sync; graph-capturable), _status,
 *      _stripe_status, _groups and _destroy as any plan does, and
 *        rs_plan_bytes   returns the sum over the stripes with r_b > 0 of
 *                        sizes[b] * (k + w_b + c_b);
 *        rs_plan_forms   reports RS_ORDER_REQUIRED + RS_ORDER_CONSECUTIVE;
 *        rs_plan_tune, rs_plan_set_orders and rs_plan_launch_ceiling behave as for a
 *        ragged plan; no bit-sliced kernel, no hiprtc compile, no tune-table entry.
 * rs_decode_dev_required is the one-shot form, as rs_decode_dev_ragged. */
#define RS_ORDER_REQUIRED 2048
int rs_plan_create_required(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                            const uint8_t* present, const uint8_t* required,
                            uint8_t* const* shards, rs_plan** out);
int rs_decode_dev_required(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                           const uint8_t* present, const uint8_t* required,
                           uint8_t* const* shards, void* stream);

/* ---- update plans: parity updated in place -------------------------
 * Upstream Update(shards, newDatashards) and EncodeIdx(dataShard, idx, parity) for
 * device-resident batches. Stripe b has sizes[b]-byte shards and k flags at changed + b*k
 * (nonzero = data shard i changed). A launch sets, for every stripe with a changed shard,
 *     parity[b*m + j] ^= sum over the changed i of P[j][i] * (old_data[b*k+i] ^ new_data[b*k+i])
 * (P the parity rows of rs_encode_matrix), reading nothing but the old and new bytes of the
 * changed shards and the parity itself: after one launch the parity is what an encode of the
 * new data gives. old_data == NULL (the whole array) is EncodeIdx mode: the launch adds
 * P[j][i] * new_data[b*k+i] for every flagged i to whatever the parity holds (upstream has
 * the caller zero it before the first shard arrives). Entries of unflagged shards are never
 * read and may be NULL, as may every pointer of a stripe with no flag; data shards are never
 * written.
 * A LAUNCH IS NOT IDEMPOTENT: it applies the delta to the parity's current bytes. A second
 * launch applies it again, which restores the parity the first launch started from.
 * The caller's contract: no parity byte of one stripe may overlap a parity byte of another
 * stripe or any source.
 * It is an ordinary plan: rs_plan_launch / _launch_timed only enqueue (no allocation, no
 * sync; graph-capturable), one launch per group of 16 parity rows, none when no stripe has a
 * flag; _groups, _destroy as for any plan, and
 *   rs_plan_bytes   returns the sum over the stripes with c_b > 0 flags of
 *                   sizes[b] * (c_b * (2, or 1 in EncodeIdx mode) + 2m);
 *   rs_plan_forms   reports RS_ORDER_UPDATE + RS_ORDER_CONSECUTIVE;
 *   rs_plan_status  reports 0 (nothing is compared);
 *   rs_plan_tune    times nothing (it never touches the parity) and fills -1,
 *                   rs_plan_set_orders accepts only -1, and the ceiling launches return
 *                   RS_E_ARG; no bit-sliced kernel, no hiprtc compile, no tune-table entry.
 * Errors, in this order: the profile (RS_E_INVALID_PROFILE, RS_E_UNSUPPORTED); a NULL
 * sizes, changed, new_data, parity or out, or batch < 1 (RS_E_ARG); sizes[b] == 0 on a stripe
 * with a flag (RS_E_NO_DATA); a flag whose new_data entry (or, with old_data, whose old_data
 * entry) is NULL, or a NULL parity entry of such a stripe (RS_E_ARG). Nothing is created on
 * an error. */
#define RS_ORDER_UPDATE 4096
int rs_plan_create_update(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                          const uint8_t* changed, const uint8_t* const* old_data,
                          const uint8_t* const* new_data, uint8_t* const* parity, rs_plan** out);

/* ---- decode-idx plans: progressive decode ---------------------------
 * Upstream DecodeIdx(dst, expectInput, input), the decode twin of EncodeIdx, for device-resident
 * batches: the k shards a decode will be fed are fixed up front, and every launch adds the
 * contribution of the shards that have arrived so far into the wanted outputs, in any order and
 * any grouping. Stripe b has sizes[b]-byte shards and, over its n = k+m shard indices, entries
 * b*n + i of three arrays:
 *   expect  (flags)    nonzero = shard i will be delivered over all calls. Exactly k must be set:
 *                      fewer is RS_E_TOO_FEW_SHARDS, more is RS_E_ARG.
 *   input   (pointers) non-NULL = shard i is delivered with this plan. An input at an index that
 *                      is not expected is RS_E_ARG.
 *   dst     (pointers) non-NULL = shard i is wanted. A dst at an expected index is RS_E_ARG. Any
 *                      index that is not expected may be wanted, data or parity, and any may be
 *                      left out: it is then neither read nor written.
 *   flags              0 = merge, RS_DECODE_IDX_STORE = store; any other bit is RS_E_ARG.
 * With V the expected indices in ascending order and C = E[w] * inv(E[V]) (E = rs_encode_matrix;
 * C's row for w is the row rs_decode_rows returns for a presence mask equal to expect), a launch
 * sets for every wanted w of every stripe that has both an input and a dst
 *     merge:  dst[w] ^= sum over the delivered v of C[w][v] * input[v]
 *     store:  dst[w]  = sum over the delivered v of C[w][v] * input[v]   (dst is neither read nor
 *                                                                        zeroed)
 * After every expected shard has been delivered once, dst holds bit for bit what a reconstruct
 * with exactly those k shards present gives -- from zeroed destinations, or when the first launch
 * stores. With expect = the data shards and dst = the parity this is EncodeIdx. A stripe with no
 * input or no wanted shard is in no launch and keeps every byte, in both modes.
 * A MERGE LAUNCH IS NOT IDEMPOTENT: it adds the terms to the destination's current bytes, and a
 * second launch adds them again, which restores what the first started from. A store launch is
 * idempotent.
 * The caller's contract: no dst byte of a stripe overlaps a dst byte of another stripe or any
 * input.
 * It is an ordinary plan: rs_plan_launch / _launch_timed only enqueue (no allocation, no sync;
 * graph-capturable), one launch per group of 16 wanted rows; _destroy as for any plan, and
 *   rs_plan_groups  returns the number of row groups, 0 when no stripe is in a launch;
 *   rs_plan_bytes   returns the sum over the stripes in the launch, with c_b delivered and r_b
 *                   wanted shards, of sizes[b] * (c_b + 2 r_b) in merge mode and
 *                   sizes[b] * (c_b + r_b) in store mode;
 *   rs_plan_forms   reports RS_ORDER_DECODE_IDX + RS_ORDER_CONSECUTIVE;
 *   rs_plan_status  reports 0 (nothing is compared);
 *   rs_plan_tune    times nothing and fills -1, rs_plan_set_orders accepts only -1, and the
 *                   ceiling launches return RS_E_ARG; no bit-sliced kernel, no hiprtc compile, no
 *                   tune-table entry.
 * Errors, in this order: the profile (RS_E_INVALID_PROFILE, RS_E_UNSUPPORTED); a NULL sizes,
 * expect, input, dst or out, batch < 1, or a flag bit other than RS_DECODE_IDX_STORE (RS_E_ARG);
 * a stripe whose expect count is not k (RS_E_TOO_FEW_SHARDS below k, RS_E_ARG above); an input at
 * an index that is not expected or a dst at one that is (RS_E_ARG); sizes[b] == 0 on a stripe with
 * both an input and a dst (RS_E_NO_DATA). Each check runs over the whole batch before the next.
 * Nothing is created on an error. */
#define RS_ORDER_DECODE_IDX 32768
int rs_plan_create_decode_idx(rs_ctx* ctx, int device, int k, int m, int batch,
                              const size_t* sizes, const uint8_t* expect,
                              const uint8_t* const* input, uint8_t* const* dst,
                              unsigned flags, rs_plan** out);

/* ---- decode-check plans: progressive Verify -------------------------
 * A decode-idx plan that also checks the shards a download fetched beyond the k expected ones,
 * so that a progressive decode ends with the Verify that upstream Decode makes (codec.go:59)
 * without keeping the k expected shards resident. sizes, expect, input, dst and the store flag are
 * those of rs_plan_create_decode_idx; a fourth array of batch * (k+m) pointers joins them:
 *   check   (pointers) non-NULL = shard i is compared. Allowed only where expect[i] == 0 and
 *                      dst[i] == NULL (RS_E_ARG otherwise). It names an S-byte syndrome
 *                      accumulator owned by the caller, under dst's overlap contract: no byte of
 *                      it overlaps a dst or check byte of another stripe or row, or any input.
 *   input   (pointers) non-NULL is allowed at an expected index, or at an index whose check entry
 *                      is non-NULL in the same call: the compared shard itself arriving. An input
 *                      at any other index is RS_E_ARG.
 *   flags              RS_DECODE_IDX_STORE and RS_DECODE_CHECK_FINAL; any other bit is RS_E_ARG.
 * Wanted rows are computed as by a decode-idx plan; a compared shard's delivery adds nothing to
 * them. With V and C as there, a launch sets for every compared j
 *     check[j] (^)= sum over the delivered expected v of C[j][v] * input[v]
 *                   ^ input[j] if shard j is delivered with this plan
 * with ^= in merge mode and = under RS_DECODE_IDX_STORE. After every expected shard and shard j
 * have been delivered once, in any order and grouping -- from a zeroed accumulator, or when the
 * first launch stores -- check[j] is shard j XOR the shard the k expected ones imply: all zero
 * exactly when shard j lies on their codeword.
 * RS_DECODE_CHECK_FINAL changes what happens to the check rows: a check row is NOT WRITTEN; every
 * byte of the value it would have received is tested, and a nonzero byte sets the stripe's status
 * word, which rs_plan_status and rs_plan_stripe_status report and clear as for every compare.
 * Wanted rows are still written. With FINAL|STORE check rows are neither read nor written and the
 * pointer only marks the index: the one-shot decode plus Verify. Under FINAL a stripe with a
 * check row is in the launch even when nothing is delivered with this plan, and the launch then
 * only scans its accumulators; without FINAL a stripe needs an input and a (wanted or check) row
 * to be in the launch. So after every expected and every compared shard has been delivered once,
 * the last launch being FINAL, dst holds a reconstruct's bytes from exactly the k expected
 * shards, and the stripe's flag is set exactly when some compared shard differs from what the
 * expected shards imply -- the flag the compare launches of a ragged plan report for
 * present = expected and compared. A compared shard that never arrives is left out by passing
 * check[j] = NULL in the final plan.
 * A NON-FINAL MERGE LAUNCH IS NOT IDEMPOTENT, for check rows as for wanted rows: a second launch
 * adds the terms again. A FINAL LAUNCH WITHOUT WANTED ROWS IS IDEMPOTENT: it writes no shard byte
 * (the status word it may set stays set until it is read).
 * An ordinary plan, as a decode-idx plan, with these differences:
 *   rs_plan_launch  a non-final plan dispatches the decode-idx kernels (a check row is an
 *                   ordinary row there), a final plan the check kernels; one launch per group of
 *                   16 rows of the wanted and compared indices in ascending order;
 *   rs_plan_bytes   a decode-idx plan's count for the delivered (compared ones included) and
 *                   wanted shards, plus per check row 2 sizes[b] in a non-final merge, sizes[b] in
 *                   a non-final store or a final merge, and nothing under FINAL|STORE;
 *   rs_plan_forms   a final plan reports RS_ORDER_DECODE_CHECK + RS_ORDER_CONSECUTIVE, a
 *                   non-final one RS_ORDER_DECODE_IDX + RS_ORDER_CONSECUTIVE;
 *   rs_plan_status  reports what the final launches since the last read flagged.
 * Errors, in rs_plan_create_decode_idx's order: the profile; a NULL sizes, expect, input, dst,
 * check or out, batch < 1, or an unknown flag bit (RS_E_ARG); the expect count; a misplaced
 * pointer -- an input at an index that is neither expected nor compared, a dst or a check at an
 * expected index, a check and a dst at one index (RS_E_ARG); sizes[b] == 0 on a stripe in the
 * launch (RS_E_NO_DATA). Each check runs over the whole batch before the next. Nothing is created
 * on an error. */
#define RS_DECODE_CHECK_FINAL 2u
#define RS_ORDER_DECODE_CHECK 65536
int rs_plan_create_decode_check(rs_ctx* ctx, int device, int k, int m, int batch,
                                const size_t* sizes, const uint8_t* expect,
                                const uint8_t* const* input, uint8_t* const* dst,
                                uint8_t* const* check, unsigned flags, rs_plan** out);

/* ---- decode-repair plans: progressive repair ------------------------
 * Not in the reference API. A final decode-check plan flags a stripe whose shards do not lie on
 * one codeword; by then its wanted rows were built from the corrupt shard. A decode-repair plan
 * is that final plan -- the same sizes, expect, input, dst and check arrays under the same
 * contracts, and it is ALWAYS FINAL -- whose launch also names the corrupt shard byte column by
 * byte column, repairs the wanted rows within the launch and hands the error values back:
 *   fix     (pointers) batch * (k+m); non-NULL is allowed at an expected or a compared index
 *                      (RS_E_ARG anywhere else). It names S bytes the caller owns. XOR in place
 *                      is the whole contract: a zeroed buffer ends up holding the shard's error
 *                      row, a buffer holding the shard as delivered ends up holding the shard
 *                      restored. Only damaged 16-byte vectors (and damaged tail bytes) are read and
 *                      written. fix[i] may equal input[i] of the same plan, a shard repaired where
 *                      it lies; otherwise dst's overlap contract applies.
 *   flags              0 (merge) or RS_DECODE_IDX_STORE; any other bit is RS_E_ARG.
 * Every row's final value is what the final decode-check launch forms (merge: the accumulator XOR
 * the computed row; store: the computed row). Per byte column the r' check values are the
 * syndromes and the correct plans' rule decides over them (locate_correct with rows = r', so a
 * verdict needs r' >= 3: with fewer every mismatching column is unexplained):
 *   expected shard V[j], value e   every wanted row r gets G[r][j] * e XORed in
 *                                  (G = E[rows] * inv(E[V])); e is XORed into fix[V[j]]'s byte
 *                                  when that pointer is given;
 *   compared shard x, value s_x    the wanted rows are unchanged; s_x is XORed into fix[x]'s byte
 *                                  when given;
 *   unexplained                    the wanted rows are stored as computed; the column is counted.
 * The wanted rows hold these values when the launch has finished on the stream. Within the
 * launch a wanted row's 16-byte vector is stored as computed first and, in a vector with a
 * repaired column, read back and stored again by the same lane: until the launch ends dst may
 * hold the unrepaired bytes, as it may hold anything while a launch writes it.
 * A check row is NOT WRITTEN. The stripe's status word is set for every stripe that had a
 * mismatching column, repaired or not, as for correct plans. The plan holds batch * (k+m+1) counts
 * that rs_plan_blame reads and clears, launches adding into them until the next read: entry i of
 * stripe b is the number of columns blamed on shard i (whether or not fix[i] was given), entry
 * k+m the number of unexplained columns.
 * A LAUNCH WITH WANTED ROWS IN MERGE MODE IS NOT IDEMPOTENT, as every merge, and a launch with a
 * fix row that finds damage is not either; A LAUNCH WITH NO WANTED AND NO FIX ROWS IS IDEMPOTENT
 * (counts and the status word accumulate until read).
 * A stripe has at most 16 rows, compared and wanted together: all syndromes and all wanted rows
 * of a column meet in one block, and the plan has one launch group.
 * An ordinary plan, as a final decode-check plan: rs_plan_launch[_timed] only enqueue
 * (graph-capturable); rs_plan_status, rs_plan_stripe_status, rs_plan_blame and rs_plan_groups as
 * on correct plans; rs_plan_bytes is the final decode-check plan's figure for the same flags (the
 * few repaired bytes are not counted); rs_plan_forms reports RS_ORDER_DECODE_REPAIR +
 * RS_ORDER_CONSECUTIVE; rs_plan_tune fills -1, rs_plan_set_orders takes -1 only and the ceiling
 * launches return RS_E_ARG.
 * Errors, in this order: the profile; a NULL sizes, expect, input, dst, check, fix or out,
 * batch < 1, or an unknown flag bit (RS_E_ARG); the expect count (RS_E_TOO_FEW_SHARDS below k,
 * RS_E_ARG above); a misplaced pointer -- rs_plan_create_decode_check's, or a fix at an index that
 * is neither expected nor compared (RS_E_ARG); a stripe with more than 16 rows
 * (RS_E_UNSUPPORTED); sizes[b] == 0 on a stripe in the launch (RS_E_NO_DATA). Each check runs
 * over the whole batch before the next. Nothing is created on an error. */
#define RS_ORDER_DECODE_REPAIR 131072
int rs_plan_create_decode_repair(rs_ctx* ctx, int device, int k, int m, int batch,
                                 const size_t* sizes, const uint8_t* expect,
                                 const uint8_t* const* input, uint8_t* const* dst,
                                 uint8_t* const* check, uint8_t* const* fix, unsigned flags,
                                 rs_plan** out);

/* ---- feed objects: one shard per launch, rows resident ---------------
 * A decode-check plan fixes its delivered set when it is created, so a download that receives its
 * shards one at a time needs a plan per arrival. A feed object fixes only what is known before the
 * first shard lands -- one stripe of S-byte shards, its k expected shards, its wanted and its
 * compared shards -- and every launch then delivers one shard, named by argument:
 *   expect  (flags)    k+m entries, exactly k set: fewer is RS_E_TOO_FEW_SHARDS, more RS_E_ARG.
 *   dst     (pointers) k+m entries, non-NULL = shard i is wanted; not at an expected index.
 *   check   (pointers) k+m entries, non-NULL = shard i is compared; not at an expected index and
 *                      not where dst is given.
 * dst[i] and check[i] name S-byte device accumulators owned by the caller, under the overlap
 * contract of decode-check plans: no byte of one overlaps another or any source. The rows are the
 * compared indices in ascending order, then the wanted indices in ascending order -- a
 * decode-repair plan's order, so a final decode-check or decode-repair plan with nothing delivered
 * can take the same pointers and close the decode. At most 16 rows (RS_E_UNSUPPORTED above).
 * rs_feed_launch(feed, idx, src, flags, stream) delivers shard idx, which must be expected or
 * compared (RS_E_ARG otherwise; also for a NULL feed or src or a flag bit other than
 * RS_DECODE_IDX_STORE). src is S bytes the device can read -- device memory or host-coherent
 * pinned memory -- at any alignment. Its effect on every row is exactly that of a non-final
 * decode-check plan with that one input, with C = E[rows] * inv(E[V]) as there:
 *     expected idx:  row (^)= C[row][idx] * src   for every row
 *     compared idx:  check[idx] (^)= src          and no other row is touched
 * with ^= for flags 0 and = under RS_DECODE_IDX_STORE. A store launch reads no row and writes
 * every row; rows other than a compared shard's own then receive zeros. So the first launch of a
 * decode stores and the later ones merge, in any order of arrival.
 * A MERGE LAUNCH IS NOT IDEMPOTENT: it adds the terms to the rows' current bytes, and a second
 * launch adds them again, which restores what the first started from. A store launch is
 * idempotent.
 * The launch only enqueues one kernel on `stream`: no allocation, no copy, no sync;
 * graph-capturable (the arguments go by value). The coefficient tables are built once, in
 * rs_feed_create, with one k x k inversion, and uploaded once.
 * Errors of rs_feed_create, in this order: the profile (RS_E_INVALID_PROFILE, RS_E_UNSUPPORTED);
 * a NULL ctx, expect, dst, check or out (RS_E_ARG); the expect count; a misplaced pointer -- a dst
 * or a check at an expected index, a check and a dst at one index (RS_E_ARG); more than 16 rows
 * (RS_E_UNSUPPORTED); S == 0 (RS_E_NO_DATA); then an unknown device (RS_E_ARG). Each check runs
 * before the next. Nothing is created on an error. */
typedef struct rs_feed rs_feed;
int rs_feed_create(rs_ctx* ctx, int device, int k, int m, size_t S, const uint8_t* expect,
                   uint8_t* const* dst, uint8_t* const* check, rs_feed** out);
int rs_feed_launch(rs_feed* feed, int idx, const uint8_t* src, unsigned flags, void* stream);
void rs_feed_destroy(rs_feed* feed);

/* ---- decode sessions: shards fed from host memory as they land -------
 * The host route over a feed object, for a download that receives its shards one at a time in
 * host memory. rs_decode_check keeps nothing on the device between calls: every arrival uploads
 * and downloads every row. A session keeps one stripe's rows -- the syndrome accumulators of the
 * compared shards and the wanted shards -- on one device from open to close, so an arrival moves
 * its own S bytes and nothing else, and builds its tables once.
 * rs_session_open: expect, want and compare are k+m flags each (nonzero = set) under
 *   rs_feed_create's rules: exactly k expected, a wanted or compared index never expected, never
 *   both, at most 16 of them together. flags: RS_SESSION_CHECK (finish flags a mismatch) or
 *   RS_SESSION_REPAIR (finish also repairs it). Allocates the rows (zeroed, at a pitch of S rounded
 *   up to 256), a stream, a ring of CALLFS_RS_SESSION_SLOTS source slots (default 3) and the feed
 *   object, on the context's next device in round-robin order. A session holds none of the
 *   context's lanes: a long download does not starve the other host calls. Errors in
 *   rs_feed_create's order, an unknown flag bit counting with the NULL arrays.
 * rs_session_feed: delivers shard idx, expected or compared, from S bytes of host memory. Calls
 *   on one session are serialised by a mutex and may come from any thread, in any order of
 *   arrival; the first feed stores, the later ones merge. It returns once `shard` may be reused,
 *   and blocks only while every slot of the ring holds a shard whose launch has not finished. A
 *   second feed of one index, an index that is neither expected nor compared, and any feed after
 *   finish are RS_E_ARG. Two routes into the one kernel, chosen by CALLFS_RS_SESSION_INPLACE_MAX
 *   (bytes per shard, read at open; default 2 MiB):
 *     in place  up to that size: the shard is copied into a host-coherent slot and the kernel
 *               reads it over PCIe; a shard inside an rs_host_alloc buffer is read where it lies,
 *               with no host copy at all, and the call then returns when the kernel has read it;
 *     staged    above it: one H2D from staging into a device slot, then the launch.
 *   rs_host_counters per feed: calls 1, launches 1, copies 0 in place and 1 staged.
 * rs_session_peek: waits for the feeds enqueued so far and copies the first len <= S bytes of
 *   the accumulator of a wanted or compared index (RS_E_ARG for any other): the partial result.
 *   Before the first feed the rows read zero.
 * rs_session_finish: RS_E_TOO_FEW_SHARDS while fewer than k expected shards have been fed; the
 *   session stays open and usable. Otherwise the decode is closed: compared shards that were
 *   never fed are left out (check = NULL in the final plan); when a compared shard was delivered
 *   one final plan runs over the resident rows with nothing delivered -- under RS_SESSION_CHECK
 *   rs_plan_create_decode_check with RS_DECODE_CHECK_FINAL and without the wanted rows, under
 *   RS_SESSION_REPAIR rs_plan_create_decode_repair -- and then the wanted rows are copied out.
 *     dst      k+m pointers: dst[i] of a wanted index receives dst_lens[i] <= S bytes (dst_lens
 *              NULL: S bytes; dst[i] NULL: skipped), so a caller joins and trims by pointing dst
 *              into its object buffer. A destination inside an rs_host_alloc buffer takes its D2H
 *              directly; the others share one D2H of the wanted rows' span.
 *     fix      RS_SESSION_REPAIR: k+m pointers or NULL; fix[i] is allowed at an expected index and
 *              at a compared index that was fed (RS_E_ARG elsewhere, and under RS_SESSION_CHECK).
 *              XOR in place, as rs_decode_repair: the device fix rows are allocated and zeroed
 *              here, and a row comes back, to be XORed into fix[i], only when the status word is
 *              set and the shard was blamed.
 *     counts   NULL or k+m+1 words as rs_plan_blame fills them (zero under RS_SESSION_CHECK).
 *   The dst bytes, the fix bytes, counts and the return value are bit for bit those of one
 *   rs_decode_check call with RS_DECODE_CHECK_FINAL | RS_DECODE_IDX_STORE (RS_SESSION_REPAIR:
 *   one rs_decode_repair call with RS_DECODE_IDX_STORE) given all delivered shards at once:
 *   RS_E_CORRUPT still delivers the wanted rows. After a finish that ran, further feeds and
 *   finishes are RS_E_ARG; peek still works.
 * rs_session_close waits for the session's stream and frees everything. */
#define RS_SESSION_CHECK 0u
#define RS_SESSION_REPAIR 1u
typedef struct rs_session rs_session;
int rs_session_open(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* expect,
                    const uint8_t* want, const uint8_t* compare, unsigned flags,
                    rs_session** out);
int rs_session_feed(rs_session* session, int idx, const uint8_t* shard);
int rs_session_peek(rs_session* session, int idx, uint8_t* out, size_t len);
int rs_session_finish(rs_session* session, uint8_t* const* dst, const size_t* dst_lens,
                      uint8_t* const* fix, uint64_t* counts);
void rs_session_close(rs_session* session);

/* ---- absorb objects: body ranges into resident parity rows -----------
 * The upload twin of a feed object. An object of L bytes under RS(k,m) has S = ceil(L / k)
 * (rs_shard_size); object byte x is byte x % S of data shard x / S, as Split lays it out. An
 * absorb object fixes k, m, S and the m parity rows: rows[j] names an S-byte device accumulator
 * owned by the caller (no byte of one overlaps another or any source), zero before the first
 * launch. At most 16 rows (RS_E_UNSUPPORTED above).
 * rs_absorb_launch(absorb, off, len, src, stream) folds the body range [off, off + len) in: src
 * is len bytes the device can read -- device memory or host-coherent pinned memory -- at any
 * alignment, body byte off + b at src[b]. Its effect is exactly
 *     rows[j][c] ^= P[j][i] * body[i * S + c]    for every fed byte (i, c) and every j
 * with P the parity rows of the encoding matrix, and nothing else: no byte of a row outside the
 * columns the range touches is read or written. When every byte of [0, L) has been fed exactly
 * once, in any order, the rows are bit for bit the parity shards rs_codec_encode writes for the
 * body; bytes L .. k*S-1 are Split's zero padding and need not be fed.
 * A LAUNCH IS NOT IDEMPOTENT: it adds the range's terms to the rows' current bytes, and a second
 * launch of the same range adds them again, which restores what the first started from. Launches
 * of disjoint ranges commute; launches on one stream, or otherwise ordered, never race.
 * The launch only enqueues one kernel on `stream`, however many shards the range covers: no
 * allocation, no copy, no sync; graph-capturable (the arguments go by value). The coefficient
 * tables are built once, in rs_absorb_create, and uploaded once.
 * Errors of rs_absorb_create, in this order: the profile (RS_E_INVALID_PROFILE,
 * RS_E_UNSUPPORTED); a NULL ctx, rows, out or row pointer (RS_E_ARG); more than 16 rows
 * (RS_E_UNSUPPORTED); S == 0 (RS_E_NO_DATA); then an unknown device (RS_E_ARG). Each check runs
 * before the next. Nothing is created on an error. rs_absorb_launch returns RS_E_ARG for a NULL
 * absorb or src, len == 0 and a range that does not lie inside [0, k*S). */
typedef struct rs_absorb rs_absorb;
int rs_absorb_create(rs_ctx* ctx, int device, int k, int m, size_t S, uint8_t* const* rows,
                     rs_absorb** out);
int rs_absorb_launch(rs_absorb* absorb, uint64_t off, uint64_t len, const uint8_t* src,
                     void* stream);
void rs_absorb_destroy(rs_absorb* absorb);

/* ---- encode sessions: the body fed from host memory as it arrives ----
 * The host route over an absorb object, for an upload whose body arrives in reads that ignore
 * shard boundaries. rs_codec_encode starts when the last body byte is in host memory and then
 * pays the H2D of k*S, the kernel and the D2H of m*S. A session keeps the m parity rows on one
 * device from open to close; every piece of the body goes up once, as it arrives, and after the
 * last byte only the D2H of m*S is left.
 * rs_encode_session_open(ctx, k, m, len, &session): an object of len bytes, S =
 *   ceil(len / k) (rs_shard_size). Allocates the rows (zeroed, at a pitch of S rounded up to 256), a
 *   stream, a ring of CALLFS_RS_SESSION_SLOTS source slots (default 3) of min(len,
 *   CALLFS_RS_ENCODE_SESSION_CHUNK) bytes each (default 4 MiB) and the absorb object, on the
 *   context's next device in round-robin order. A session holds none of the context's lanes.
 *   Errors, in this order: the profile; a NULL ctx or session (RS_E_ARG); len == 0
 *   (RS_E_SHORT_DATA, as rs_codec_encode); m > 16 (RS_E_UNSUPPORTED).
 * rs_encode_session_feed(session, off, bytes, n): body bytes [off, off + n) from host memory.
 *   Calls on one session are serialised by a mutex and may come from any thread, in any order.
 *   A FEED IS NOT IDEMPOTENT, so every body byte is fed exactly once: a range that is empty,
 *   reaches past len, overlaps anything fed before or comes after a finish is RS_E_ARG, and
 *   nothing is launched for it. It returns once `bytes` may be reused and blocks only while every
 *   slot of the ring holds a piece whose launch has not finished. A feed larger than a slot is cut
 *   into slot-sized pieces, one launch each. Per piece one of three routes into the one kernel,
 *   chosen by CALLFS_RS_SESSION_INPLACE_MAX (bytes per piece, read at open; default 2 MiB):
 *     in place  up to that size: the piece is copied into a host-coherent slot and the kernel
 *               reads it over PCIe;
 *     direct    up to that size and inside an rs_host_alloc buffer: read where it lies, with no
 *               host copy at all; the call then returns when the kernel has read it;
 *     staged    above it: one H2D from staging into a device slot, then the launch.
 *   rs_host_counters: calls 1 per feed; per piece launches 1, copies 0 in place and direct and 1
 *   staged.
 * rs_encode_session_peek(session, j, out, n): waits for the feeds so far and copies the first
 *   n <= S bytes of parity row j, 0 <= j < m (RS_E_ARG otherwise): the parity of the body with
 *   every byte not yet fed taken as zero.
 * rs_encode_session_finish(session, parity, &shard_size): RS_E_SHORT_DATA while [0, len) is not
 *   covered; the session stays open and usable. Otherwise it waits for the stream and copies the
 *   m rows out, S bytes each into parity[j]; a destination inside an rs_host_alloc buffer takes
 *   its D2H directly, the others share one D2H through pinned staging. *shard_size (may be NULL)
 *   receives S. The bytes are those rs_codec_encode writes for the body. A finish may be repeated:
 *   it changes nothing. Feeds after it are RS_E_ARG. The data shards are the caller's body; the
 *   session never copies them back.
 * rs_encode_session_close waits for the session's stream and frees everything. */
typedef struct rs_encode_session rs_encode_session;
int rs_encode_session_open(rs_ctx* ctx, int k, int m, size_t len, rs_encode_session** out);
int rs_encode_session_feed(rs_encode_session* session, uint64_t off, const uint8_t* bytes,
                           size_t n);
int rs_encode_session_peek(rs_encode_session* session, int j, uint8_t* out, size_t n);
int rs_encode_session_finish(rs_encode_session* session, uint8_t* const* parity,
                             size_t* shard_size);
void rs_encode_session_close(rs_encode_session* session);

/* ---- locate plans: which shard is corrupt --------------------------
 * Not in the reference API. Every other plan tells that a stripe's compared shards mismatch; a
 * locate plan tells where. sizes, present and shards as for rs_plan_create_ragged, but present
 * == NULL means every shard of every stripe is present. Nothing is written: a launch reads, per
 * stripe, the first k present shards and the next r' = min(present - k, 16) present shards,
 * recomputes the latter from the former and, for every byte column in which they differ,
 * decides from the r' differences (the syndromes) which one shard explains them:
 *   - one compared shard differs alone: that shard is blamed;
 *   - every compared shard differs, consistently with one error in one of the k read shards:
 *     that shard is blamed;
 *   - anything else, and every mismatch of a stripe with r' = 1: the column is unexplained.
 * Over the k + r' examined shards a column with one corrupt byte is blamed on exactly that
 * shard, and a column with 2..r'-1 corrupt bytes is never blamed on anybody; with r' or more
 * corrupt bytes a column can be misattributed or look clean. Present shards past the 16th
 * compared one are neither read nor blamed. A stripe with exactly k present shards has no row
 * and is in no launch; its counts and flag stay 0.
 * rs_plan_blame synchronises `stream` and copies out batch * (k+m+1) counts: counts[b*(k+m+1) +
 * i] is the number of byte columns of stripe b blamed on shard i, and entry k+m of a stripe
 * its unexplained columns. It then clears them, as rs_plan_stripe_status clears the flags.
 * LAUNCHES ACCUMULATE until the next read: a plan launched twice before a read reports every
 * count doubled. RS_E_ARG for NULL or for a plan that is not a locate plan.
 * It is an ordinary plan otherwise: rs_plan_launch / _launch_timed only enqueue (no allocation,
 * no sync; graph-capturable); _status and _stripe_status report a flag for every stripe with a
 * nonzero syndrome; _destroy as for any plan, and
 *   rs_plan_groups  returns 1, or 0 when no stripe has a row;
 *   rs_plan_bytes   returns the sum over the stripes with a row of sizes[b] * (k + r'_b);
 *   rs_plan_forms   reports RS_ORDER_LOCATE + RS_ORDER_CONSECUTIVE;
 *   rs_plan_tune, rs_plan_set_orders and rs_plan_launch_ceiling behave as for a ragged plan;
 *   no bit-sliced kernel, no hiprtc compile, no tune-table entry.
 * Errors are those of rs_plan_create_ragged. */
#define RS_ORDER_LOCATE 8192
int rs_plan_create_locate(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                          const uint8_t* present, uint8_t* const* shards, rs_plan** out);
int rs_plan_blame(rs_plan* plan, void* stream, uint64_t* counts);

/* ---- locate and heal, host memory -----------------------------------
 * rs_locate / rs_locate_batch: the locate plan's counts for stripes in host memory; shards and
 * lens as for rs_verify / rs_reconstruct_batch (lens 0 = missing; nothing is written), counts
 * as for rs_plan_blame (k+m+1 words per stripe, written for every stripe, zero where nothing ran).
 * Argument and shard checks and status[b] follow rs_reconstruct_batch with verify != 0:
 * RS_E_NO_DATA, RS_E_SHARD_SIZE, RS_E_TOO_FEW_SHARDS, RS_E_ARG (a NULL present shard), and
 * RS_E_CORRUPT for a stripe with any mismatching column -- its counts say where. rs_locate
 * returns that status; rs_locate_batch RS_OK or the first nonzero status in stripe order, and
 * call-level errors as rs_reconstruct_batch. A stripe with exactly k present shards has zero
 * counts and is RS_OK without device work; a call of such stripes alone reaches no device. The
 * calls take the staged ragged pipeline (a chunk: one H2D, one launch, one D2H of status words
 * and counts) whatever memory the buffers are in; a stripe above CALLFS_RS_CHUNK_BYTES is cut
 * into column parts whose counts are added up. rs_host_counters counts them like the others.
 * rs_heal_batch: rs_reconstruct_batch with verify that repairs what it can. (a) Reconstruct and
 * verify; stripes that come back RS_OK are done, healed all 0. (b) Each RS_E_CORRUPT stripe is
 * located over its original presence; B = the shards with a nonzero count. It is healed only
 * if no column is unexplained, B is not empty and present - |B| >= k + 1, so that a compared
 * shard is left to confirm with. (c) B and the originally missing shards are rebuilt from the
 * others and the rest verified again: clean -> status[b] = RS_OK, healed[b*(k+m) + i] = 1 for
 * i in B, every lens entry S; otherwise RS_E_CORRUPT. Present shards outside B are never
 * written; on RS_E_CORRUPT the bytes of the originally missing shards and of B are
 * unspecified. Other status values and the return value as rs_reconstruct_batch.
 * rs_codec_decode_heal: rs_codec_decode with that heal in place of the bare Verify failure;
 * healed receives k+m flags. Error precedence, join and trim are rs_codec_decode's. */
int rs_locate(rs_ctx* ctx, int k, int m, const uint8_t* const* shards, const size_t* lens,
              uint64_t* counts);
int rs_locate_batch(rs_ctx* ctx, int k, int m, int batch, const uint8_t* const* shards,
                    const size_t* lens, uint64_t* counts, int* status);
int rs_heal_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards, size_t* lens,
                  uint8_t* healed, int* status);
int rs_codec_decode_heal(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                         uint8_t* out, int64_t original_size, uint8_t* healed);

/* ---- two corrupt shards per byte column ----------------------------
 * The _ex calls are their siblings above with one more argument, max_errors: how many corrupt
 * shards a byte column may be blamed on.
 *   max_errors == 1: exactly the sibling (which is this call with 1);
 *   max_errors == 2: a pair plan. A pattern that compares r' >= 4 shards also explains a column
 *     in which two of the k + r' examined shards are corrupt: the column counts once for EACH of
 *     the two shards, so a stripe's counts may add up to more than its columns. Columns with one
 *     corrupt byte get exactly the verdict of max_errors == 1. For e corrupt examined bytes in a
 *     column: e = 2 is blamed on exactly those two shards; 3 <= e <= r'-2 is unexplained (an
 *     empty range at r' = 4); e >= r'-1 may be misattributed or look clean -- at r' = 4 that
 *     starts at three errors, which max_errors == 1 still reports as unexplained. Patterns
 *     with r' < 4 behave as with max_errors == 1.
 *   max_errors < 1 returns RS_E_ARG (with the NULL and count checks), max_errors > 2
 *   RS_E_UNSUPPORTED (after them); both before any device work.
 * rs_plan_blame, the counts layout (k+m+1 words per stripe), rs_plan_forms (RS_ORDER_LOCATE +
 * RS_ORDER_CONSECUTIVE) and every other plan call are unchanged. The heal rule is unchanged
 * too: B = the shards with a nonzero count, and a stripe is healed when nothing is unexplained,
 * B is not empty and present - |B| >= k + 1; the second verify stays the backstop against a
 * misattributed column. */
int rs_plan_create_locate_ex(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                             const uint8_t* present, uint8_t* const* shards, int max_errors,
                             rs_plan** out);
int rs_locate_ex(rs_ctx* ctx, int k, int m, const uint8_t* const* shards, const size_t* lens,
                 uint64_t* counts, int max_errors);
int rs_locate_batch_ex(rs_ctx* ctx, int k, int m, int batch, const uint8_t* const* shards,
                       const size_t* lens, uint64_t* counts, int* status, int max_errors);
int rs_heal_batch_ex(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards, size_t* lens,
                     uint8_t* healed, int* status, int max_errors);
int rs_codec_decode_heal_ex(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                            uint8_t* out, int64_t original_size, uint8_t* healed, int max_errors);

/* ---- correct plans: repair corrupt bytes in place --------------------
 * A correct plan is a locate plan (max_errors 1: the same arguments, errors in the same order,
 * the same tables byte for byte) whose launch repairs what it blames: in a mismatching byte
 * column that one shard explains, the error value is XORed into that shard's byte. THE SHARD
 * POINTERS ARE WRITTEN THROUGH, the k read shards included, so `shards` must name writable
 * memory. A column is corrected only in a stripe that compares r' >= 3 shards: two syndromes
 * make the verdict and at least one more must confirm it (a corrected column is a codeword, so
 * no later verify could catch a miscorrection). With r' < 3 nothing is written and every
 * mismatching column is unexplained. For r' >= 3 and e corrupt examined bytes in a column:
 *   e = 0: clean; e = 1: that byte is restored exactly; 2 <= e <= r'-1: untouched and
 *   unexplained; e >= r': may be miscorrected.
 * rs_plan_blame reads (and clears) batch * (k+m+1) counts: counts[b*(k+m+1) + i] is the number
 * of bytes of shard i of stripe b the launches changed, entry k+m the columns left mismatching.
 * A second launch over repaired data changes nothing and adds only to that last entry.
 * _status and _stripe_status flag every stripe that HAD a mismatch, corrected or not.
 * rs_plan_launch / _launch_timed only enqueue (no allocation, no sync; graph-capturable);
 * rs_plan_groups and rs_plan_bytes are the locate plan's (the few bytes written are not
 * counted); rs_plan_forms reports RS_ORDER_CORRECT + RS_ORDER_CONSECUTIVE; rs_plan_tune,
 * rs_plan_set_orders and rs_plan_launch_ceiling behave as for a locate plan. Missing shards are
 * neither read nor rebuilt. Pair correction (max_errors 2) is not built.
 * rs_correct / rs_correct_batch: the same for stripes in host memory, on the staged ragged
 * pipeline like rs_locate_batch (checks, their order and the column parts of large stripes are
 * that call's). After a chunk's launch the counts come back first and only the (stripe, shard)
 * rows with a nonzero count are copied back into the caller's shards: a call over clean stripes
 * copies no shard byte back. counts as for rs_plan_blame. status[b] is RS_OK when nothing
 * mismatched or every mismatching column was corrected, RS_E_CORRUPT when a column is left
 * (bytes already corrected stay corrected). A stripe with exactly k present shards is RS_OK
 * with zero counts and reaches no device.
 * rs_codec_decode_correct: rs_codec_decode's checks, then one rs_correct over the present
 * shards, then the ordinary decode (reconstruct, verify, join, trim), whose result it returns:
 * RS_E_CORRUPT exactly when the decode still fails after the correction. corrected receives
 * k+m flags: 1 for a shard with a nonzero count. */
#define RS_ORDER_CORRECT 16384
int rs_plan_create_correct(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                           const uint8_t* present, uint8_t* const* shards, rs_plan** out);
int rs_correct(rs_ctx* ctx, int k, int m, uint8_t* const* shards, const size_t* lens,
               uint64_t* counts);
int rs_correct_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                     const size_t* lens, uint64_t* counts, int* status);
int rs_codec_decode_correct(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                            uint8_t* out, int64_t original_size, uint8_t* corrected);

/* ---- ShardChecksum on device-resident shards (codec.go:81-84; §8(f) of SURVEY.md) ----
 * SHA-256 of `count` messages already in HBM, one digest per message written to
 * `digests` (device memory, 32*count bytes, FIPS 180-4 byte order — hex-encode it for
 * the Go string). msgs/lens are HOST arrays of device pointers and byte lengths.
 * SHA-256 is serial within a message, so this pays off only in batches of many shards
 * (scrub, device-resident pipelines); a single request's checksums stay on the CPU.
 * rs_sha256_plan_* upload the message table once; rs_sha256_dev is the one-shot form
 * (synchronous on `stream`). */
typedef struct rs_hash_plan rs_hash_plan;
int  rs_sha256_plan_create(rs_ctx* ctx, int device, const uint8_t* const* msgs,
                           const uint64_t* lens, int count, rs_hash_plan** out);
int  rs_sha256_plan_launch(rs_hash_plan* plan, uint8_t* digests, void* stream);
void rs_sha256_plan_destroy(rs_hash_plan* plan);
int  rs_sha256_dev(rs_ctx* ctx, int device, const uint8_t* const* msgs, const uint64_t* lens,
                   int count, uint8_t* digests, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CALLFS_RS_H */
