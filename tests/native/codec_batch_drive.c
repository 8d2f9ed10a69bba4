/* Drives rs_codec_encode_batch / rs_codec_decode_batch as the cgo shim does
 * (go/erasure/codec_rocm.go EncodeBatch / DecodeBatch): C-malloc'd pointer, lens, size and
 * status arrays over separately allocated buffers, nil shards as lens 0, bodies split in
 * place in a buffer with room for all n shards.
 *
 * Without a HIP device (rs_init -> RS_E_HIP) only the argument and status paths that return
 * before any device work run, against a context pointer the library must not dereference on
 * them (tests/test_native_codec_batch.py builds this with -fsanitize=address,undefined on the
 * CPU): call-level errors leave status[] alone, and a batch in which no object is runnable
 * reports every object's status and writes no buffer. With a device the same binary also
 * runs mixed batches, each object checked against the C oracle (oracle/rs_oracle.c, linked
 * as the checker only).
 *
 * usage: codec_batch_drive [gpu]   ("gpu": fail unless a device is present) */
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
  /* ---- encode ---- */
  {
    uint8_t** data = (uint8_t**)malloc(sizeof(uint8_t*) * B);
    uint8_t** outp = (uint8_t**)malloc(sizeof(uint8_t*) * B);
    size_t* lens = (size_t*)malloc(sizeof(size_t) * B);
    size_t* caps = (size_t*)malloc(sizeof(size_t) * B);
    size_t* ss = (size_t*)malloc(sizeof(size_t) * B);
    int* st = (int*)malloc(sizeof(int) * B);
    for (int b = 0; b < B; b++) {
      data[b] = (uint8_t*)malloc(K * S);
      outp[b] = (uint8_t*)malloc(N * S);
      memset(data[b], b + 1, K * S);
      memset(outp[b], SENTINEL, N * S);
      lens[b] = K * S - 1;
      caps[b] = N * S;
      ss[b] = 7;
      st[b] = UNSET;
    }
    /* call-level: profile first, then NULL arrays and a negative count; status untouched */
    CHECK(rs_codec_encode_batch(ctx, 0, M, B, (const uint8_t* const*)data, lens, outp, caps, ss, st) == RS_E_INVALID_PROFILE);
    CHECK(rs_codec_encode_batch(ctx, K, 0, B, (const uint8_t* const*)data, lens, outp, caps, ss, st) == RS_E_INVALID_PROFILE);
    CHECK(rs_codec_encode_batch(ctx, 200, 100, B, (const uint8_t* const*)data, lens, outp, caps, ss, st) == RS_E_UNSUPPORTED);
    CHECK(rs_codec_encode_batch(NULL, K, M, B, (const uint8_t* const*)data, lens, outp, caps, ss, st) == RS_E_ARG);
    CHECK(rs_codec_encode_batch(ctx, K, M, -1, (const uint8_t* const*)data, lens, outp, caps, ss, st) == RS_E_ARG);
    CHECK(rs_codec_encode_batch(ctx, K, M, B, NULL, lens, outp, caps, ss, st) == RS_E_ARG);
    CHECK(rs_codec_encode_batch(ctx, K, M, B, (const uint8_t* const*)data, NULL, outp, caps, ss, st) == RS_E_ARG);
    CHECK(rs_codec_encode_batch(ctx, K, M, B, (const uint8_t* const*)data, lens, NULL, caps, ss, st) == RS_E_ARG);
    CHECK(rs_codec_encode_batch(ctx, K, M, B, (const uint8_t* const*)data, lens, outp, NULL, ss, st) == RS_E_ARG);
    CHECK(rs_codec_encode_batch(ctx, K, M, B, (const uint8_t* const*)data, lens, outp, caps, NULL, st) == RS_E_ARG);
    CHECK(rs_codec_encode_batch(ctx, K, M, B, (const uint8_t* const*)data, lens, outp, caps, ss, NULL) == RS_E_ARG);
    for (int b = 0; b < B; b++) CHECK(st[b] == UNSET && ss[b] == 7);
    /* an empty batch is fine, whatever the arrays */
    CHECK(rs_codec_encode_batch(ctx, K, M, 0, NULL, NULL, NULL, NULL, NULL, NULL) == RS_OK);
    /* no runnable object: an empty one (Split -> ErrShortData), a nil body, a short buffer */
    uint8_t* body0 = data[0];
    uint8_t* body1 = data[1];
    lens[0] = 0;
    data[1] = NULL;
    caps[2] = N * S - 1;
    CHECK(rs_codec_encode_batch(ctx, K, M, B, (const uint8_t* const*)data, lens, outp, caps, ss, st) == RS_E_SHORT_DATA);
    CHECK(st[0] == RS_E_SHORT_DATA && st[1] == RS_E_ARG && st[2] == RS_E_ARG);
    for (int b = 0; b < B; b++) CHECK(ss[b] == 7 && all_bytes(outp[b], N * S, SENTINEL));
    /* a nil shards_out, and an empty object whose pointers are nil too */
    data[1] = body1;
    uint8_t* out1 = outp[1];
    outp[1] = NULL;
    data[0] = NULL;
    CHECK(rs_codec_encode_batch(ctx, K, M, 2, (const uint8_t* const*)data, lens, outp, caps, ss, st) == RS_E_SHORT_DATA);
    CHECK(st[0] == RS_E_SHORT_DATA && st[1] == RS_E_ARG);
    outp[1] = out1;
    data[0] = body0;
    for (int b = 0; b < B; b++) {
      CHECK(all_bytes(outp[b], N * S, SENTINEL));
      free(data[b]);
      free(outp[b]);
    }
    free(st); free(ss); free(caps); free(lens); free(outp); free(data);
  }
  /* ---- decode ---- */
  {
    uint8_t** sh = (uint8_t**)malloc(sizeof(uint8_t*) * B * N);
    size_t* lens = (size_t*)malloc(sizeof(size_t) * B * N);
    size_t* lens0 = (size_t*)malloc(sizeof(size_t) * B * N);
    uint8_t** outp = (uint8_t**)malloc(sizeof(uint8_t*) * B);
    int64_t* sizes = (int64_t*)malloc(sizeof(int64_t) * B);
    int* st = (int*)malloc(sizeof(int) * B);
    for (int b = 0; b < B; b++) {
      for (int i = 0; i < N; i++) {
        sh[b * N + i] = (uint8_t*)malloc(S);
        memset(sh[b * N + i], SENTINEL, S);
        lens[b * N + i] = S;
      }
      outp[b] = (uint8_t*)malloc(K * S);
      memset(outp[b], SENTINEL, K * S);
      sizes[b] = (int64_t)(K * S - 3);
      st[b] = UNSET;
    }
    CHECK(rs_codec_decode_batch(ctx, 0, M, B, sh, lens, outp, sizes, st) == RS_E_INVALID_PROFILE);
    CHECK(rs_codec_decode_batch(ctx, 200, 100, B, sh, lens, outp, sizes, st) == RS_E_UNSUPPORTED);
    CHECK(rs_codec_decode_batch(NULL, K, M, B, sh, lens, outp, sizes, st) == RS_E_ARG);
    CHECK(rs_codec_decode_batch(ctx, K, M, -2, sh, lens, outp, sizes, st) == RS_E_ARG);
    CHECK(rs_codec_decode_batch(ctx, K, M, B, NULL, lens, outp, sizes, st) == RS_E_ARG);
    CHECK(rs_codec_decode_batch(ctx, K, M, B, sh, NULL, outp, sizes, st) == RS_E_ARG);
    CHECK(rs_codec_decode_batch(ctx, K, M, B, sh, lens, NULL, sizes, st) == RS_E_ARG);
    CHECK(rs_codec_decode_batch(ctx, K, M, B, sh, lens, outp, NULL, st) == RS_E_ARG);
    CHECK(rs_codec_decode_batch(ctx, K, M, B, sh, lens, outp, sizes, NULL) == RS_E_ARG);
    for (int b = 0; b < B; b++) CHECK(st[b] == UNSET);
    CHECK(rs_codec_decode_batch(ctx, K, M, 0, NULL, NULL, NULL, NULL, NULL) == RS_OK);
    /* no runnable object, in the order of the checks: object 0 has a short shard beside too
       few (size before count), object 1 lacks m+1 shards, object 2 has a nil buffer behind a
       present length (and would be insufficient: ARG comes first) */
    for (int i = 0; i < M + 1; i++) lens[0 * N + i] = lens[1 * N + i] = 0;
    lens[0 * N + N - 1] = S - 1;
    uint8_t* keep = sh[2 * N + 1];
    sh[2 * N + 1] = NULL;
    sizes[2] = (int64_t)(K * S + 1);
    memcpy(lens0, lens, sizeof(size_t) * B * N);
    CHECK(rs_codec_decode_batch(ctx, K, M, B, sh, lens, outp, sizes, st) == RS_E_SHARD_SIZE);
    CHECK(st[0] == RS_E_SHARD_SIZE && st[1] == RS_E_TOO_FEW_SHARDS && st[2] == RS_E_ARG);
    CHECK(memcmp(lens, lens0, sizeof(size_t) * B * N) == 0);
    /* every entry nil; a negative size; a nil out with a positive size */
    sh[2 * N + 1] = keep;
    for (int i = 0; i < N; i++) lens[0 * N + i] = 0;
    for (int i = 0; i < M + 1; i++) lens[1 * N + i] = S;
    sizes[1] = -1;
    uint8_t* out2 = outp[2];
    outp[2] = NULL;
    sizes[2] = 1;
    memcpy(lens0, lens, sizeof(size_t) * B * N);
    CHECK(rs_codec_decode_batch(ctx, K, M, B, sh, lens, outp, sizes, st) == RS_E_NO_DATA);
    CHECK(st[0] == RS_E_NO_DATA && st[1] == RS_E_ARG && st[2] == RS_E_ARG);
    outp[2] = out2;
    CHECK(memcmp(lens, lens0, sizeof(size_t) * B * N) == 0);
    for (int b = 0; b < B; b++) {
      CHECK(all_bytes(outp[b], K * S, SENTINEL));
      for (int i = 0; i < N; i++) CHECK(all_bytes(sh[b * N + i], S, SENTINEL));
    }
    for (int b = 0; b < B; b++) {
      for (int i = 0; i < N; i++) free(sh[b * N + i]);
      free(outp[b]);
    }
    free(st); free(sizes); free(outp); free(lens0); free(lens); free(sh);
  }
}

static uint32_t lcg(uint32_t* s) {
  *s = *s * 1664525u + 1013904223u;
  return *s >> 24;
}

/* One mixed batch: objects of the given lengths, odd ones split in place in a body with room
 * for n shards (the shim's BodyBuffer), even ones into a separate buffer; then every object
 * decoded in one call from separately allocated shards, object b having lost shards
 * b % n and (b % 2 ? none : (b + 3) % n), object 1 with a flipped byte in a compared shard
 * (m >= 2 throughout). */
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
  for (int b = 0; b < B; b++) {
    const size_t S = (L[b] + (size_t)k - 1) / (size_t)k;
    uint32_t seed = (uint32_t)(L[b] * 31u + (unsigned)b);
    orig[b] = (uint8_t*)malloc(L[b]);
    for (size_t i = 0; i < L[b]; i++) orig[b][i] = (uint8_t)lcg(&seed);
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
  CHECK(rs_codec_encode_batch(ctx, k, m, B, (const uint8_t* const*)data, lens, outp, caps, ss, st) == RS_OK);
  for (int b = 0; b < B; b++) {
    const size_t S = (L[b] + (size_t)k - 1) / (size_t)k;
    CHECK(st[b] == RS_OK && ss[b] == S);
    CHECK(memcmp(outp[b], want[b], S * (size_t)n) == 0);
    CHECK(outp[b][S * (size_t)n] == SENTINEL);
    if (b % 2 == 0) CHECK(memcmp(data[b], orig[b], L[b]) == 0);
  }
  /* decode */
  uint8_t** sh = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)B * (size_t)n);
  size_t* sl = (size_t*)malloc(sizeof(size_t) * (size_t)B * (size_t)n);
  uint8_t** obj = (uint8_t**)malloc(sizeof(uint8_t*) * (size_t)B);
  int64_t* sizes = (int64_t*)malloc(sizeof(int64_t) * (size_t)B);
  const int corrupt = B > 1 ? 1 : -1; /* an odd object: it loses one shard */
  for (int b = 0; b < B; b++) {
    const size_t S = ss[b];
    const int lost0 = b % n, lost1 = b % 2 ? -1 : (b + 3) % n;
    for (int i = 0; i < n; i++) {
      uint8_t* p = (uint8_t*)malloc(S + 1);
      p[S] = SENTINEL;
      if (i == lost0 || i == lost1) {
        memset(p, SENTINEL, S);
        sl[b * n + i] = 0;
      } else {
        memcpy(p, want[b] + S * (size_t)i, S);
        sl[b * n + i] = S;
      }
      sh[b * n + i] = p;
    }
    if (b == corrupt) { /* the last present shard is compared: fewer than m are lost */
      int i = n - 1;
      while (i == lost0 || i == lost1) i--;
      sh[b * n + i][S / 2] ^= 0x40;
    }
    obj[b] = (uint8_t*)malloc(L[b] + 1);
    memset(obj[b], SENTINEL, L[b] + 1);
    sizes[b] = (int64_t)L[b];
    st[b] = UNSET;
  }
  const int rc = rs_codec_decode_batch(ctx, k, m, B, sh, sl, obj, sizes, st);
  CHECK(rc == (corrupt >= 0 ? RS_E_CORRUPT : RS_OK));
  for (int b = 0; b < B; b++) {
    const size_t S = ss[b];
    const int bad = b == corrupt;
    CHECK(st[b] == (bad ? RS_E_CORRUPT : RS_OK));
    if (!bad) CHECK(memcmp(obj[b], orig[b], L[b]) == 0);
    CHECK(obj[b][L[b]] == SENTINEL);
    for (int i = 0; i < n; i++) {
      CHECK(sl[b * n + i] == S && sh[b * n + i][S] == SENTINEL);
      if (!bad) CHECK(memcmp(sh[b * n + i], want[b] + S * (size_t)i, S) == 0);
      free(sh[b * n + i]);
    }
    free(obj[b]);
    if (b % 2 == 0) free(data[b]);
    free(outp[b]); free(orig[b]); free(want[b]);
  }
  free(sizes); free(obj); free(sl); free(sh);
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
    printf(fails ? "codec_batch_drive FAILED (%d)\n" : "codec_batch_drive ok (argument paths, no device)\n", fails);
    return fails != 0;
  }
  if (rc != RS_OK) {
    printf("rs_init failed: %s\n", rs_strerror(rc));
    return 2;
  }
  argument_paths(ctx);
  const size_t small[] = {2, 1, 4097, 63, 40000, 9, 123457, 4096};  /* one dispatch in place */
  device_batch(ctx, 4, 2, small, 8);
  device_batch(ctx, 10, 4, small, 8);
  const size_t large[] = {(3u << 20) + 5, 700, (1u << 20) - 1, 64};  /* staged, several sizes */
  device_batch(ctx, 10, 4, large, 4);
  const size_t same[] = {50000, 50000, 50000};                      /* the uniform pipeline */
  device_batch(ctx, 16, 4, same, 3);
  rs_shutdown(ctx);
  printf(fails ? "codec_batch_drive FAILED (%d)\n" : "codec_batch_drive ok (device round trips)\n", fails);
  return fails != 0;
}
