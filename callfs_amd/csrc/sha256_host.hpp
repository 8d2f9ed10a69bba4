// SHA-256 of one message on the CPU (FIPS 180-4): erasure.ShardChecksum (codec.go:81-84) for
// the shards a checksummed codec batch hashes on the host, one message per copy-pool task
// (DESIGN.md §7.7). The x86 SHA extensions where the processor has them, portable C++
// elsewhere; both are bit-exact with sha256.hip. Plain C++ with no HIP dependence:
// tests/native/sums_host_test.cpp checks it against its own software SHA-256.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace callfs {

namespace sha256_detail {

alignas(16) constexpr uint32_t kK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4,
    0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe,
    0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f,
    0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7,
    0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc,
    0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b,
    0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116,
    0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7,
    0xc67178f2};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

inline void blocks_portable(uint32_t (&st)[8], const uint8_t* p, size_t nblk) {
  for (; nblk; --nblk, p += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = static_cast<uint32_t>(p[4 * i]) << 24 | static_cast<uint32_t>(p[4 * i + 1]) << 16 |
             static_cast<uint32_t>(p[4 * i + 2]) << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kK[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      h = g; g = f; f = e; e = d + t1;
      d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
    st[4] += e; st[5] += f; st[6] += g; st[7] += h;
  }
}

#if defined(__x86_64__)
// Four rounds per step: sha256rnds2 twice on the {ABEF, CDGH} halves of the state, the
// message schedule through sha256msg1 / sha256msg2 (Intel's SHA extensions programming
// reference).
__attribute__((target("sha,sse4.1,ssse3"))) inline void blocks_shani(uint32_t (&st)[8], const uint8_t* p,
                                                                   size_t nblk) {
  const __m128i bswap = _mm_set_epi64x(0x0c0d0e0f08090a0bLL, 0x0405060700010203LL);
  __m128i t = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(&st[0])), 0xB1);  // CDAB
  __m128i s1 = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(&st[4])), 0x1B);  // EFGH
  __m128i s0 = _mm_alignr_epi8(t, s1, 8);  // ABEF
  s1 = _mm_blend_epi16(s1, t, 0xF0);       // CDGH
  for (; nblk; --nblk, p += 64) {
    const __m128i save0 = s0, save1 = s1;
    __m128i m[4];
#pragma GCC unroll 16
    for (int g = 0; g < 16; ++g) {
      if (g < 4) {
        m[g] = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p + 16 * g)), bswap);
      } else {
        // W[g] from W[g-4], W[g-3], W[g-2], W[g-1]
        const __m128i x = _mm_add_epi32(_mm_sha256msg1_epu32(m[g & 3], m[(g + 1) & 3]),
                                        _mm_alignr_epi8(m[(g + 3) & 3], m[(g + 2) & 3], 4));
        m[g & 3] = _mm_sha256msg2_epu32(x, m[(g + 3) & 3]);
      }
      __m128i wk = _mm_add_epi32(m[g & 3], _mm_load_si128(reinterpret_cast<const __m128i*>(&kK[4 * g])));
      s1 = _mm_sha256rnds2_epu32(s1, s0, wk);
      wk = _mm_shuffle_epi32(wk, 0x0E);
      s0 = _mm_sha256rnds2_epu32(s0, s1, wk);
    }
    s0 = _mm_add_epi32(s0, save0);
    s1 = _mm_add_epi32(s1, save1);
  }
  t = _mm_shuffle_epi32(s0, 0x1B);   // FEBA
  s1 = _mm_shuffle_epi32(s1, 0xB1);  // DCHG
  _mm_storeu_si128(reinterpret_cast<__m128i*>(&st[0]), _mm_blend_epi16(t, s1, 0xF0));  // DCBA
  _mm_storeu_si128(reinterpret_cast<__m128i*>(&st[4]), _mm_alignr_epi8(s1, t, 8));     // HGFE
}
#endif

inline bool has_shani() {
#if defined(__x86_64__)
  static const bool v = __builtin_cpu_supports("sha") && __builtin_cpu_supports("sse4.1") &&
                        __builtin_cpu_supports("ssse3");
  return v;
#else
  return false;
#endif
}

inline void blocks(uint32_t (&st)[8], const uint8_t* p, size_t nblk, bool portable) {
#if defined(__x86_64__)
  if (!portable && has_shani()) return blocks_shani(st, p, nblk);
#endif
  (void)portable;
  blocks_portable(st, p, nblk);
}

}  // namespace sha256_detail

// out: the 32 digest bytes in FIPS order. portable = true keeps to the C++ rounds (the test
// compares both).
inline void sha256_host(const uint8_t* msg, size_t len, uint8_t* out, bool portable = false) {
  uint32_t st[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                    0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const size_t full = len / 64, rem = len - full * 64;
  sha256_detail::blocks(st, msg, full, portable);
  // tail: the remaining bytes, 0x80, zeros, the 64-bit big-endian bit length (1 or 2 blocks)
  uint8_t tail[128] = {0};
  if (rem) std::memcpy(tail, msg + full * 64, rem);
  tail[rem] = 0x80;
  const size_t nblk = rem < 56 ? 1 : 2;
  const uint64_t bits = static_cast<uint64_t>(len) * 8;
  for (int i = 0; i < 8; ++i) tail[nblk * 64 - 1 - static_cast<size_t>(i)] = static_cast<uint8_t>(bits >> (8 * i));
  sha256_detail::blocks(st, tail, nblk, portable);
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) out[4 * i + j] = static_cast<uint8_t>(st[i] >> (24 - 8 * j));
}

}  // namespace callfs
