/* Drives rs_codec_encode_batch_sums / rs_codec_decode_batch_sums as the cgo shim does
 * (go/erasure/codec_rocm_sums.go EncodeBatchSums / DecodeBatchSums): C-malloc'd pointer, lens,
 * size and status arrays over separately allocated buffers, one digest array of batch*n*32
 * bytes and one flag array of batch*n bytes, nil shards as lens 0, bodies split in place in a
 * buffer with room for all n shards, a mismatching shard rebuilt inside its own buffer.
 *
 * Without a HIP device (rs_init -> RS_E_HIP) only the argument and status paths that return
 * before any device work run, against a context pointer the library must not dereference on
 * them: call-level errors leave status[], digests and bad alone, and a batch in which no
 * object is runnable reports every object's status, writes no digest and zeroes bad. With a
 * device the same binary also runs mixed batches: shards against the C oracle
 * (oracle/rs_oracle.c, linked as the checker only), the digest of an "abc" shard against the
 * FIPS 180-4 vector, a clean decode against the digests the encode returned, then one with a
 * flipped byte, a wrong digest and an object left with too few good shards.
 *
 * usage: sums_drive [gpu]   ("gpu": fail unless a device is present) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "callfs_rs.h"

int orc_encode(int k, int m, size_t S, const uint8_t* const* data, uint8_t* const* parity);

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
      ++fails;                                                \
    }                                                         \
  } while (0)

#define SENTINEL 0xA5
#define UNSET (-12345)

static int all_bytes(const uint8_t* p, size_t n, uint8_t v) {
  for (size_t i = 0; i < n; i++)
    if (p[i] != v) return 0;
  return 1;
}

/* Paths that return before any device work. */
static void argument_paths(rs_ctx* ctx) {
  enum { K = 4, M = 2, N = 6, B = 3 };
  const size_t S = 100;
  uint8_t** data = (uint8_t**)malloc(sizeof(uint8_t*) * B);
  uint8_t** outp = (uint8_t**)malloc(sizeof(uint8_t*) * B);
  uint8_t** sh = (uint8_t**)malloc(sizeof(uint8_t*) * B * N);
  size_t* lens = (size_t*)malloc(sizeof(size_t) * B);
  size_t* sl = (size_t*)malloc(sizeof(size_t) * B * N);
  size_t* caps = (size_t*)malloc(sizeof(size_t) * B);
  size_t* ss = (size_t*)malloc(sizeof(size_t) * B);
  int64_t* sizes = (int64_t*)malloc(sizeof(int64_t) * B);
  int* st = (int*)malloc(sizeof(int) * B);
  uint8_t* dig = (uint8_t*)malloc(B * N * 32);
  uint8_t* bad = (uint8_t*)malloc(B * N);
  memset(dig, SENTINEL, B * N * 32);
  memset(bad, SENTINEL, B * N);
  for (int b = 0; b < B; b++) {
    data[b] = (uint8_t*)malloc(K * S);
    outp[b] = (uint8_t*)malloc(N * S);
    memset(data[b], b + 1, K * S);
    memset(outp[b], SENTINEL, N * S);
    lens[b] = K * S - 1;
    caps[b] = N * S;
    ss[b] = 7;
    sizes[b] = (int64_t)(K * S);
    st[b] = UNSET;
    for (int i = 0; i < N; i++) {
      sh[b * N + i] = (uint8_t*)malloc(S);
      memset(sh[b * N + i], SENTINEL, S);
      sl[b * N + i] = S;
    }
  }
  const uint8_t* const* cdata = (const uint8_t* const*)data;
  /* call-level: profile first, then NULL arrays and a negative count */
  CHECK(rs_codec_encode_batch_sums(ctx, 0, M, B, cdata, lens, outp, caps, ss, dig, st) == RS_E_INVALID_PROFILE);
  CHECK(rs_codec_encode_batch_sums(ctx, 200, 100, B, cdata, lens, outp, caps, ss, dig, st) == RS_E_UNSUPPORTED);
  CHECK(rs_codec_encode_batch_sums(NULL, K, M, B, cdata, lens, outp, caps, ss, dig, st) == RS_E_ARG);
  CHECK(rs_codec_encode_batch_sums(ctx, K, M, -1, cdata, lens, outp, caps, ss, dig, st) == RS_E_ARG);
  CHECK(rs_codec_encode_batch_sums(ctx, K, M, B, NULL, lens, outp, caps, ss, dig, st) == RS_E_ARG);
  CHECK(rs_codec_encode_batch_sums(ctx, K, M, B, cdata, lens, outp, caps, ss, NULL, st) == RS_E_ARG);
  CHECK(rs_codec_encode_batch_sums(ctx, K, M, B, cdata, lens, outp, caps, ss, dig, NULL) == RS_E_ARG);
  CHECK(rs_codec_encode_batch_sums(ctx, K, M, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == RS_OK);
  CHECK(rs_codec_decode_batch_sums(ctx, 0, M, B, sh, sl, dig, outp, sizes, bad, st) == RS_E_INVALID_PROFILE);
  CHECK(rs_codec_decode_batch_sums(ctx, 200, 100, B, sh, sl, dig, outp, sizes, bad, st) == RS_E_UNSUPPORTED);
  CHECK(rs_codec_decode_batch_sums(NULL, K, M, B, sh, sl, dig, outp, sizes, bad, st) == RS_E_ARG);
  CHECK(rs_codec_decode_batch_sums(ctx, K, M, -2, sh, sl, dig, outp, sizes, bad, st) == RS_E_ARG);
  CHECK(rs_codec_decode_batch_sums(ctx, K, M, B, NULL, sl, dig, outp, sizes, bad, st) == RS_E_ARG);
  CHECK(rs_codec_decode_batch_sums(ctx, K, M, B, sh, sl, NULL, outp, sizes, bad, st) == RS_E_ARG);
  CHECK(rs_codec_decode_batch_sums(ctx, K, M, B, sh, sl, dig, outp, sizes, NULL, st) == RS_E_ARG);
  CHECK(rs_codec_decode_batch_sums(ctx, K, M, B, sh, sl, dig, outp, sizes, bad, NULL) == RS_E_ARG);
  CHECK(rs_codec_decode_batch_sums(ctx, K, M, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == RS_OK);
  for (int b = 0; b < B; b++) CHECK(st[b] == UNSET && ss[b] == 7);
  CHECK(all_bytes(dig, B * N * 32, SENTINEL) && all_bytes(bad, B * N, SENTINEL));
  /* no runnable object: every status is the object's own, no digest is written */
  lens[0] = 0;        /* empty object */
  caps[1] = N * S - 1; /* too small a buffer (S of K*S - 1 bytes is S) */
  uint8_t* data2 = data[2];
  data[2] = NULL;     /* (restored below) */
  CHECK(rs_codec_encode_batch_sums(ctx, K, M, B, cdata, lens, outp, caps, ss, dig, st) == RS_E_SHORT_DATA);
  CHECK(st[0] == RS_E_SHORT_DATA && st[1] == RS_E_ARG && st[2] == RS_E_ARG);
  CHECK(all_bytes(dig, B * N * 32, SENTINEL));
  for (int b = 0; b < B; b++) CHECK(all_bytes(outp[b], N * S, SENTINEL));
  /* decode: a wrong length, too few shards, nothing present; bad is zeroed, nothing else moves */
  sl[0 * N + 2] = S - 1;
  for (int i = 0; i < 3; i++) sl[1 * N + i] = 0;
  for (int i = 0; i < N; i++) sl[2 * N + i] = 0;
  for (int b = 0; b < B; b++) st[b] = UNSET;
  CHECK(rs_codec_decode_batch_sums(ctx, K, M, B, sh, sl, dig, outp, sizes, bad, st) == RS_E_SHARD_SIZE);
  CHECK(st[0] == RS_E_SHARD_SIZE && st[1] == RS_E_TOO_FEW_SHARDS && st[2] == RS_E_NO_DATA);
  CHECK(all_bytes(bad, B * N, 0));
  CHECK(sl[0 * N + 2] == S - 1 && sl[1 * N + 0] == 0 && sl[1 * N + 3] == S);
  for (int b = 0; b < B; b++) {
    CHECK(all_bytes(outp[b], N * S, SENTINEL));
    for (int i = 0; i < N; i++) CHECK(all_bytes(sh[b * N + i], S, SENTINEL));
  }
  data[2] = data2;
  for (int b = 0; b < B; b++) {
    for (int i = 0; i < N; i++) free(sh[b * N + i]);
    free(data[b]);
    free(outp[b]);
  }
  free(bad); free(dig); free(st); free(sizes); free(ss); free(caps); free(sl); free(lens);
  free(sh); free(outp); free(data);
}

static uint32_t lcg(uint32_t* s) {
  *s = *s * 1664525u + 1013904223u;
  return *s >> 24;
}

/* One mixed batch through EncodeBatchSums, then DecodeBatchSums twice over separately
 * allocated shards: clean (object b has lost shard b % n), then with object 0's shard
 * (b0) flipped in its last byte, object 1's digest of a good shard wrong and object 2 left
 * with k - 1 good shards. */
static void device_batch(rs_ctx* ctx, int k, int m, const size_t* L, int B) {
  const int n = k + m;
  uint8_t** data = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)B);
  uint8_t** outp = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)B);
  uint8_t** orig = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)B);
  uint8_t** want = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)B); /* n*S: the codeword */
  size_t* lens = (size_t*)malloc(sizeof(size_t) * (size_t)B);
  size_t* caps = (size_t*)malloc(sizeof(size_t) * (size_t)B);
  size_t* ss = (size_t*)malloc(sizeof(size_t) * (size_t)B);
  int* st = (int*)malloc(sizeof(int) * (size_t)B);
  uint8_t* dig = (uint8_t*)malloc((size_t)B * (size_t)n * 32 + 1);
  memset(dig, SENTINEL, (size_t)B * (size_t)n * 32 + 1);
  for (int b = 0; b < B; b++) {
    const size_t S = (L[b] + (size_t)k - 1) / (size_t)k;
    uint32_t seed = (uint32_t)(L[b] * 31u + (unsigned)b);
    orig[b] = (uint8_t*)malloc(L[b]);
    for (size_t i = 0; i < L[b]; i++) orig[b][i] = L[b] == 3u * (size_t)k ? (uint8_t)("abc"[i % 3]) : (uint8_t)lcg(&seed);
    want[b] = (uint8_t*)calloc(S * (size_t)n, 1);
    memcpy(want[b], orig[b], L[b]);
    const uint8_t** din = (const uint8_t**)malloc(sizeof(uint8_t*) * (size_t)k);
    uint8_t** pout = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)m);
    for (int i = 0; i < k; i++) din[i] = want[b] + S * (size_t)i;
    for (int j = 0; j < m; j++) pout[j] = want[b] + S * (size_t)(k + j);
    CHECK(orc_encode(k, m, S, din, pout) == 0);
    free(pout); free(din);
    outp[b] = (uint8_t*)malloc(S * (size_t)n + 1);
    memset(outp[b], SENTINEL, S * (size_t)n + 1);
    if (b % 2) { /* in place */
      memcpy(outp[b], orig[b], L[b]);
      data[b] = outp[b];
    } else {
      data[b] = (uint8_t*)malloc(L[b]);
      memcpy(data[b], orig[b], L[b]);
    }
    lens[b] = L[b];
    caps[b] = S * (size_t)n;
    ss[b] = 0;
    st[b] = UNSET;
  }
  CHECK(rs_codec_encode_batch_sums(ctx, k, m, B, (const uint8_t* const*)data, lens, outp, caps, ss, dig, st) == RS_OK);
  CHECK(dig[(size_t)B * (size_t)n * 32] == SENTINEL);
  static const uint8_t abc[32] = {0xba, 0x78, 0x16, 0xbf, 0x8f, 0x01, 0xcf, 0xea, 0x41, 0x41, 0x40,
                                  0xde, 0x5d, 0xae, 0x22, 0x23, 0xb0, 0x03, 0x61, 0xa3, 0x96, 0x17,
                                  0x7a, 0x9c, 0xb4, 0x10, 0xff, 0x61, 0xf2, 0x00, 0x15, 0xad};
  for (int b = 0; b < B; b++) {
    const size_t S = (L[b] + (size_t)k - 1) / (size_t)k;
    CHECK(st[b] == RS_OK && ss[b] == S);
    CHECK(memcmp(outp[b], want[b], S * (size_t)n) == 0);
    CHECK(outp[b][S * (size_t)n] == SENTINEL);
    if (L[b] == 3u * (size_t)k) /* every data shard is "abc": SHA-256("abc"), FIPS 180-4 */
      for (int i = 0; i < k; i++) CHECK(memcmp(dig + ((size_t)b * (size_t)n + (size_t)i) * 32, abc, 32) == 0);
  }
  /* decode, three rounds */
  uint8_t** sh = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)B * (size_t)n);
  size_t* sl = (size_t*)malloc(sizeof(size_t) * (size_t)B * (size_t)n);
  uint8_t** obj = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)B);
  int64_t* sizes = (int64_t*)malloc(sizeof(int64_t) * (size_t)B);
  uint8_t* bad = (uint8_t*)malloc((size_t)B * (size_t)n + 1);
  uint8_t* expect = (uint8_t*)malloc((size_t)B * (size_t)n * 32);
  for (int round = 0; round < 2; round++) {
    memcpy(expect, dig, (size_t)B * (size_t)n * 32);
    memset(bad, SENTINEL, (size_t)B * (size_t)n + 1);
    const int hurt = round == 1;
    for (int b = 0; b < B; b++) {
      const size_t S = ss[b];
      for (int i = 0; i < n; i++) {
        uint8_t* p = (uint8_t*)malloc(S + 1);
        p[S] = SENTINEL;
        if (i == b % n) {
          memset(p, SENTINEL, S);
          sl[b * n + i] = 0;
        } else {
          memcpy(p, want[b] + S * (size_t)i, S);
          sl[b * n + i] = S;
        }
        sh[b * n + i] = p;
      }
      obj[b] = (uint8_t*)malloc(L[b] + 1);
      memset(obj[b], SENTINEL, L[b] + 1);
      sizes[b] = (int64_t)L[b];
      st[b] = UNSET;
    }
    /* object b has lost shard b % n; the shards named below are present */
    const int flip = 1;                         /* object 0: shard 1 */
    const int wrong = n - 1;                    /* object 1: its last shard */
    if (hurt) {
      sh[0 * n + flip][ss[0] - 1] ^= 0x01;
      if (B > 1) expect[((size_t)1 * (size_t)n + (size_t)wrong) * 32 + 31] ^= 0x80;
      /* object 2 (lost shard 2): m more shards go bad, k - 1 good ones are left */
      for (int j = 0; B > 2 && j < m; j++) sh[2 * n + 3 + j][0] ^= 0xFF;
    }
    const int rc = rs_codec_decode_batch_sums(ctx, k, m, B, sh, sl, expect, obj, sizes, bad, st);
    CHECK(rc == (hurt && B > 2 ? RS_E_TOO_FEW_SHARDS : RS_OK));
    CHECK(bad[(size_t)B * (size_t)n] == SENTINEL);
    for (int b = 0; b < B; b++) {
      const size_t S = ss[b];
      const int refused = hurt && b == 2;
      CHECK(st[b] == (refused ? RS_E_TOO_FEW_SHARDS : RS_OK));
      if (!refused) CHECK(memcmp(obj[b], orig[b], L[b]) == 0);
      else CHECK(all_bytes(obj[b], L[b], SENTINEL));
      CHECK(obj[b][L[b]] == SENTINEL);
      for (int i = 0; i < n; i++) {
        const int is_bad = hurt && ((b == 0 && i == flip) || (b == 1 && i == wrong) ||
                                    (b == 2 && i >= 3 && i < 3 + m));
        CHECK(bad[b * n + i] == (is_bad ? 1 : 0));
        CHECK(sh[b * n + i][S] == SENTINEL);
        if (refused) { /* as given: lens, the lost shard's buffer, the damaged bytes */
          CHECK(sl[b * n + i] == (i == b % n ? 0 : S));
          if (i == b % n) CHECK(all_bytes(sh[b * n + i], S, SENTINEL));
          else if (is_bad) CHECK(sh[b * n + i][0] == (uint8_t)(want[b][S * (size_t)i] ^ 0xFF));
          else CHECK(memcmp(sh[b * n + i], want[b] + S * (size_t)i, S) == 0);
        } else {
          CHECK(sl[b * n + i] == S);
          CHECK(memcmp(sh[b * n + i], want[b] + S * (size_t)i, S) == 0); /* healed in its own buffer */
        }
        free(sh[b * n + i]);
      }
      free(obj[b]);
    }
  }
  for (int b = 0; b < B; b++) {
    if (b % 2 == 0) free(data[b]);
    free(outp[b]); free(orig[b]); free(want[b]);
  }
  free(expect); free(bad); free(sizes); free(obj); free(sl); free(sh); free(dig);
  free(st); free(ss); free(caps); free(lens); free(want); free(orig); free(outp); free(data);
}

int main(int argc, char** argv) {
  const int need_gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
  rs_ctx* ctx = NULL;
  const int rc = rs_init(&ctx, 0);
  if (rc == RS_E_HIP && !need_gpu) {
    /* No device: a stand-in handle; these paths must return before touching it. */
    static char opaque[64];
    argument_paths((rs_ctx*)opaque);
    printf(fails ? "sums_drive FAILED (%d)\n" : "sums_drive ok (argument paths, no device)\n", fails);
    return fails != 0;
  }
  if (rc != RS_OK) {
    printf("rs_init failed: %s\n", rs_strerror(rc));
    return 2;
  }
  argument_paths(ctx);
  const size_t mixed[] = {12, 1, 4097, 63, 40000, 9, 123457, 4096};  /* 12 = 3 * k at RS(4,2) */
  device_batch(ctx, 4, 2, mixed, 8);
  const size_t mixed10[] = {30, 700, 4097, 64, 1u << 20};            /* 30 = 3 * k at RS(10,4) */
  device_batch(ctx, 10, 4, mixed10, 5);
  const size_t same[] = {50000, 50000, 50000};                      /* one size and mask: still ragged */
  device_batch(ctx, 16, 4, same, 3);
  rs_shutdown(ctx);
  printf(fails ? "sums_drive FAILED (%d)\n" : "sums_drive ok (device round trips)\n", fails);
  return fails != 0;
}
