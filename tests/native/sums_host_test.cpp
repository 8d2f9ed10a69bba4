// The host side of the checksummed codec batches (callfs_amd/csrc/sums_host.hpp,
// sha256_host.hpp, copy_pool.hpp's each()) on the CPU, built with g++
// -fsanitize=address,undefined by tests/test_native_sums.py and run directly:
//  - sha256_host, with the processor's SHA instructions (where it has them) and in portable
//    C++, against the software SHA-256 below: the FIPS 180-4 vectors, every length 0..300
//    and lengths around 4 KiB, 64 KiB and 300,000, at every alignment 0..15, with the bytes
//    around the message poisoned;
//  - the host-hash route: digest tasks write 32 bytes at (object * n + shard) * 32 and
//    nothing else, check tasks set exactly the flags of the shards that differ, with 1 and
//    with 8 pool threads;
//  - the follow-up run's bookkeeping (SumsRerun): exactly the objects that ran and have a
//    mismatch, in order, with the bad shards' lengths zero and every pointer in place; a
//    stand-in for the plain decode path (admission by count, lengths set to S) shows that
//    an object left with fewer than k good shards keeps the lengths it came with and the
//    others get theirs back, and that objects without a mismatch are not touched.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sums_host.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// FIPS 180-4 as written in the standard, byte at a time: the reference of this test.
struct SoftSha {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  uint8_t buf[64];
  size_t fill = 0;
  uint64_t total = 0;
  static uint32_t rr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  static uint32_t K(int i) {
    // the first 32 bits of the fractional parts of the cube roots of the first 64 primes
    static uint32_t k[64];
    static bool init = false;
    if (!init) {
      int count = 0;
      for (int p = 2; count < 64; ++p) {
        bool prime = true;
        for (int d = 2; d * d <= p; ++d) prime &= p % d != 0;
        if (!prime) continue;
        // cube root by bisection on 80-bit arithmetic
        long double lo = 1, hi = 8;
        for (int it = 0; it < 200; ++it) {
          const long double mid = (lo + hi) / 2;
          if (mid * mid * mid < p) lo = mid; else hi = mid;
        }
        const long double frac = lo - static_cast<long double>(static_cast<int>(lo));
        k[count++] = static_cast<uint32_t>(frac * 4294967296.0L);
      }
      init = true;
    }
    return k[i];
  }
  void block() {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(buf[4 * i]) << 24 | uint32_t(buf[4 * i + 1]) << 16 | uint32_t(buf[4 * i + 2]) << 8 | buf[4 * i + 3];
    for (int i = 16; i < 64; ++i)
      w[i] = w[i - 16] + (rr(w[i - 15], 7) ^ rr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
             (rr(w[i - 2], 17) ^ rr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    uint32_t v[8];
    std::memcpy(v, h, sizeof v);
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = v[7] + (rr(v[4], 6) ^ rr(v[4], 11) ^ rr(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) + K(i) + w[i];
      const uint32_t t2 = (rr(v[0], 2) ^ rr(v[0], 13) ^ rr(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
      for (int j = 7; j > 0; --j) v[j] = v[j - 1];
      v[4] += t1;
      v[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i) h[i] += v[i];
  }
  void put(uint8_t b) {
    buf[fill++] = b;
    if (fill == 64) {
      block();
      fill = 0;
    }
  }
  void digest(const uint8_t* p, size_t n, uint8_t* out) {
    for (size_t i = 0; i < n; ++i) put(p[i]);
    total = static_cast<uint64_t>(n) * 8;
    put(0x80);
    while (fill != 56) put(0);
    for (int i = 7; i >= 0; --i) put(static_cast<uint8_t>(total >> (8 * i)));
    for (int i = 0; i < 8; ++i)
      for (int j = 0; j < 4; ++j) out[4 * i + j] = static_cast<uint8_t>(h[i] >> (24 - 8 * j));
  }
};

void soft(const uint8_t* p, size_t n, uint8_t* out) { SoftSha().digest(p, n, out); }

std::string hex(const uint8_t* d) {
  static const char* x = "0123456789abcdef";
  std::string s;
  for (int i = 0; i < 32; ++i) {
    s.push_back(x[d[i] >> 4]);
    s.push_back(x[d[i] & 15]);
  }
  return s;
}

void test_sha() {
  uint8_t d[32];
  soft(reinterpret_cast<const uint8_t*>("abc"), 3, d);
  CHECK(hex(d) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
  soft(nullptr, 0, d);
  CHECK(hex(d) == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
  const char* two = "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq";
  soft(reinterpret_cast<const uint8_t*>(two), 56, d);
  CHECK(hex(d) == "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1");

  std::mt19937 rng(7);
  std::vector<size_t> lens;
  for (size_t n = 0; n <= 300; ++n) lens.push_back(n);
  for (size_t n : {4095u, 4096u, 4097u, 4099u, 65535u, 65536u, 65537u, 300000u}) lens.push_back(n);
  for (size_t n : lens) {
    const size_t align = n % 16;
    std::vector<uint8_t> buf(n + 64, 0xA5);
    uint8_t* msg = buf.data() + 16 + align;
    for (size_t i = 0; i < n; ++i) msg[i] = static_cast<uint8_t>(rng());
    uint8_t want[32], got[34];
    soft(msg, n, want);
    for (bool portable : {false, true}) {
      got[0] = got[33] = 0x5A;
      sha256_host(msg, n, got + 1, portable);
      CHECK(std::memcmp(got + 1, want, 32) == 0);
      CHECK(got[0] == 0x5A && got[33] == 0x5A);
    }
  }
}

void test_tasks(CopyPool& pool) {
  const int n = 6, objects = 37;
  std::mt19937 rng(11);
  std::vector<std::vector<uint8_t>> shards(static_cast<size_t>(objects) * n);
  std::vector<int> obj(objects);
  for (int b = 0; b < objects; ++b) {
    obj[b] = b;
    const size_t S = b == 5 ? 300000 : 1 + rng() % 700;
    for (int i = 0; i < n; ++i) {
      shards[static_cast<size_t>(b) * n + i].resize(S);
      for (uint8_t& x : shards[static_cast<size_t>(b) * n + i]) x = static_cast<uint8_t>(rng());
    }
  }
  // digests: every second object is hashed, the others' entries keep the sentinel
  std::vector<uint8_t> digests(static_cast<size_t>(objects) * n * 32, 0xEE);
  SumsCall enc;
  enc.mode = SumsMode::kDigest;
  enc.n = n;
  enc.obj = obj.data();
  enc.digests = digests.data();
  std::vector<SumsTask> tasks;
  for (int b = 0; b < objects; b += 2)
    for (int i = 0; i < n; ++i) {
      const auto& s = shards[static_cast<size_t>(b) * n + i];
      tasks.push_back(sums_task(enc, b, i, s.data(), s.size()));
    }
  run_sums_tasks(pool, tasks);
  for (int b = 0; b < objects; ++b)
    for (int i = 0; i < n; ++i) {
      const uint8_t* got = &digests[(static_cast<size_t>(b) * n + i) * 32];
      uint8_t want[32];
      const auto& s = shards[static_cast<size_t>(b) * n + i];
      soft(s.data(), s.size(), want);
      if (b % 2 == 0) CHECK(std::memcmp(got, want, 32) == 0);
      else
        for (int x = 0; x < 32; ++x) CHECK(got[x] == 0xEE);
    }
  // checks: full digests everywhere, then some shards and some expected digests damaged
  for (int b = 0; b < objects; ++b)
    for (int i = 0; i < n; ++i) {
      const auto& s = shards[static_cast<size_t>(b) * n + i];
      soft(s.data(), s.size(), &digests[(static_cast<size_t>(b) * n + i) * 32]);
    }
  std::vector<uint8_t> want_bad(static_cast<size_t>(objects) * n, 0), bad(want_bad.size(), 0x77);
  for (int t = 0; t < 20; ++t) {
    const size_t at = rng() % want_bad.size();
    if (want_bad[at]) continue;
    want_bad[at] = 1;
    if (t % 3 == 0) digests[at * 32 + rng() % 32] ^= 0x10;  // a wrong expected digest
    else shards[at][t % 2 ? shards[at].size() - 1 : 0] ^= 1;  // a flipped first or last byte
  }
  SumsCall dec;
  dec.mode = SumsMode::kCheck;
  dec.n = n;
  dec.obj = obj.data();
  dec.expected = digests.data();
  dec.bad = bad.data();
  tasks.clear();
  for (int b = 0; b < objects; ++b)
    for (int i = 0; i < n; ++i) {
      const auto& s = shards[static_cast<size_t>(b) * n + i];
      tasks.push_back(sums_task(dec, b, i, s.data(), s.size()));
    }
  run_sums_tasks(pool, tasks);
  CHECK(bad == want_bad);
}

void test_rerun() {
  const int k = 4, m = 2, n = 6, batch = 9;
  const size_t S = 130;
  std::vector<std::vector<uint8_t>> bufs(static_cast<size_t>(batch) * n, std::vector<uint8_t>(S, 1));
  std::vector<uint8_t*> shards;
  for (auto& b : bufs) shards.push_back(b.data());
  std::vector<size_t> lens(static_cast<size_t>(batch) * n, S);
  std::vector<std::vector<uint8_t>> outs(batch, std::vector<uint8_t>(500));
  std::vector<uint8_t*> out;
  std::vector<int64_t> sizes;
  for (int b = 0; b < batch; ++b) {
    out.push_back(outs[b].data());
    sizes.push_back(400 + b);
  }
  std::vector<size_t> ran(batch, S);
  std::vector<int> status(batch, 0);
  std::vector<uint8_t> bad(static_cast<size_t>(batch) * n, 0);
  // object 1: one bad shard; 3: two bad; 4: two missing and one bad (too few left);
  // 6: refused at admission (did not run) with a stale flag that must be ignored; 8: m bad
  bad[1 * n + 2] = 1;
  bad[3 * n + 0] = bad[3 * n + 5] = 1;
  lens[4 * n + 1] = lens[4 * n + 4] = 0;
  bad[4 * n + 3] = 1;
  ran[6] = 0;
  status[6] = RS_E_SHARD_SIZE;
  bad[6 * n + 1] = 1;
  bad[8 * n + 4] = bad[8 * n + 5] = 1;
  const std::vector<size_t> lens0 = lens;
  SumsRerun again(n, batch, ran.data(), bad.data(), shards.data(), lens.data(), out.data(), sizes.data());
  CHECK((again.objs == std::vector<int>{1, 3, 4, 8}));
  CHECK(again.count() == 4 && again.shards.size() == 4u * n && again.lens.size() == 4u * n);
  for (size_t j = 0; j < again.objs.size(); ++j) {
    const size_t b = static_cast<size_t>(again.objs[j]);
    CHECK(again.out[j] == out[b] && again.sizes[j] == sizes[b]);
    for (int i = 0; i < n; ++i) {
      CHECK(again.shards[j * n + i] == shards[b * n + i]);
      CHECK(again.lens[j * n + i] == (bad[b * n + i] ? 0 : lens0[b * n + i]));
    }
  }
  // the plain decode path's part: admission by count, lengths of the objects that run set to S
  for (size_t j = 0; j < again.objs.size(); ++j) {
    int present = 0;
    for (int i = 0; i < n; ++i) present += again.lens[j * n + i] != 0;
    if (present < k) {
      again.status[j] = RS_E_TOO_FEW_SHARDS;
      continue;
    }
    for (int i = 0; i < n; ++i) again.lens[j * n + i] = S;
    again.status[j] = j == 1 ? RS_E_CORRUPT : RS_OK;
  }
  again.finish(n, lens.data(), status.data(),
               [](int st) { return st == RS_OK || st == RS_E_CORRUPT || st == RS_E_INSUFFICIENT; });
  CHECK(status[1] == RS_OK && status[3] == RS_E_CORRUPT && status[4] == RS_E_TOO_FEW_SHARDS && status[8] == RS_OK);
  CHECK(status[0] == 0 && status[2] == 0 && status[5] == 0 && status[6] == RS_E_SHARD_SIZE && status[7] == 0);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < n; ++i) {
      const bool reran = b == 1 || b == 3 || b == 8;
      CHECK(lens[static_cast<size_t>(b) * n + i] == (reran ? S : lens0[static_cast<size_t>(b) * n + i]));
    }
  // nothing to run again
  std::vector<uint8_t> none(bad.size(), 0);
  CHECK(SumsRerun(n, batch, ran.data(), none.data(), shards.data(), lens.data(), out.data(), sizes.data()).count() == 0);
  (void)m;
}

}  // namespace

int main() {
  test_sha();
  setenv("CALLFS_RS_COPY_THREADS", "1", 1);
  {
    CopyPool one;
    test_tasks(one);
  }
  setenv("CALLFS_RS_COPY_THREADS", "8", 1);
  {
    CopyPool eight;
    test_tasks(eight);
    // each(): every index exactly once
    std::vector<std::atomic<int>> hits(1000);
    for (auto& h : hits) h = 0;
    eight.each(hits.size(), [&](size_t i) { hits[i].fetch_add(1); });
    for (auto& h : hits) CHECK(h == 1);
    eight.each(0, [&](size_t) { CHECK(false); });
  }
  test_rerun();
  std::printf("sums_host_test ok%s\n", sha256_detail::has_shani() ? " (sha extensions)" : " (portable)");
  return 0;
}
