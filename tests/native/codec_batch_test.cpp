// The per-object plan of the codec-level batch calls (callfs_amd/csrc/codec_batch.hpp) on
// the CPU, built with g++ -fsanitize=address,undefined by
// tests/test_native_codec_batch_plan.py. For k in {1, 3, 4, 10, 16, 255} and object lengths
// around every edge (1, 2, k-1, k, k+1, 16k +- 1, 16k, 8192k +- 1, a seeded large value):
//   - S, the full shards and the pad equal upstream Split's definition;
//   - split_prepare + split_row give the pipeline the zero-padded object as its k input rows,
//     for disjoint buffers, an in-place object and buffers that overlap partly, and write
//     nothing at or beyond k * S of shards_out;
//   - the tee spans of a disjoint encode, taken at column cuts of 8,192 bytes as the
//     pipeline's column parts take them, cover [0, full * S) of shards_out exactly once and
//     nothing else, so shards_out ends up holding the padded object;
//   - the join spans of a decode at the same cuts, for original sizes 0, 1, len - 1, len,
//     k * S, k * S + 1 and far beyond, cover [0, min(original_size, k * S)) of `out` exactly
//     once and nothing else (parity rows give none), and `out` receives the object's bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "codec_batch.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed (k=%d len=%zu)\n", __FILE__, __LINE__, #c, \
                   g_k, g_len);                                         \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

int g_k = 0;
size_t g_len = 0;
constexpr size_t kCut = 8192;
constexpr int kParity = 2;
constexpr uint8_t kFill = 0xEE;

std::vector<uint8_t> random_bytes(size_t n, std::mt19937& rng) {
  std::vector<uint8_t> v(n);
  for (auto& x : v) x = static_cast<uint8_t>(rng());
  return v;
}

// What the pipeline does with an object's input rows: every row in column parts of kCut
// bytes, each copied to `staged` (k rows of S) and teed through `tee`. hits counts the tee's
// writes per byte of its target.
void stage_rows(const SplitPlan& p, const uint8_t* data, uint8_t* shards_out, const Join& tee,
                std::vector<uint8_t>& staged, std::vector<uint8_t>& hits) {
  for (int i = 0; i < p.k; ++i) {
    const uint8_t* row = split_row(p, data, shards_out, i);
    for (size_t col = 0; col < p.S; col += kCut) {
      const size_t w = std::min(kCut, p.S - col);
      std::memcpy(&staged[p.S * i + col], row + col, w);
      const auto t = join_span(&tee, i, col, w);
      if (!t.first) {
        CHECK(t.second == 0);
        continue;
      }
      CHECK(t.second >= 1 && t.second <= w);
      CHECK(t.first == tee.out + p.S * i + col);
      std::memcpy(t.first, row + col, t.second);
      for (size_t x = 0; x < t.second; ++x) ++hits[static_cast<size_t>(t.first - tee.out) + x];
    }
  }
}

void check_encode(int k, size_t len, std::mt19937& rng) {
  const int n = k + kParity;
  SplitPlan p = split_plan(k, len);
  // the definition: the smallest S with k * S >= len; the shards wholly inside the object
  CHECK(p.k == k && p.len == len);
  CHECK(p.S * k >= len && (p.S - 1) * k < len);
  CHECK(p.full <= static_cast<size_t>(k) && p.full * p.S <= len);
  CHECK(p.full == static_cast<size_t>(k) || (p.full + 1) * p.S > len);
  CHECK(p.pad == p.S * k - len);
  const std::vector<uint8_t> data = random_bytes(len, rng);
  std::vector<uint8_t> want(p.S * k, 0);  // the padded object
  std::memcpy(want.data(), data.data(), len);

  // disjoint buffers
  {
    std::vector<uint8_t> so(p.S * n, kFill), staged(p.S * k, 0x11), hits(p.S * n, 0);
    SplitPlan q = p;
    split_prepare(q, n, data.data(), so.data());
    CHECK(q.rows_from_data == p.full);
    for (int i = 0; i < k; ++i) {
      const uint8_t* row = split_row(q, data.data(), so.data(), i);
      CHECK(row == (static_cast<size_t>(i) < p.full ? data.data() : so.data()) + p.S * i);
    }
    // before the pipeline: the partial shard and the pad are in place, nothing else is
    for (size_t x = 0; x < p.S * n; ++x)
      CHECK(so[x] == (x >= p.full * p.S && x < p.S * k ? want[x] : kFill));
    const Join tee = split_tee(q, so.data());
    CHECK(tee.out == so.data() && tee.len == p.full * p.S && tee.S == p.S && tee.k == k);
    stage_rows(q, data.data(), so.data(), tee, staged, hits);
    CHECK(staged == want);
    for (size_t x = 0; x < p.S * n; ++x) CHECK(hits[x] == (x < p.full * p.S ? 1 : 0));
    CHECK(std::memcmp(so.data(), want.data(), want.size()) == 0);
    for (size_t x = p.S * k; x < p.S * n; ++x) CHECK(so[x] == kFill);
  }
  // in place: the object at the start of its shard buffer
  {
    std::vector<uint8_t> so(p.S * n, kFill), staged(p.S * k, 0x11), hits(p.S * n, 0);
    std::memcpy(so.data(), data.data(), len);
    SplitPlan q = p;
    split_prepare(q, n, so.data(), so.data());
    CHECK(q.rows_from_data == 0);
    const Join tee = split_tee(q, so.data());
    CHECK(tee.len == 0);
    stage_rows(q, so.data(), so.data(), tee, staged, hits);
    CHECK(staged == want);
    for (size_t x = 0; x < p.S * n; ++x) CHECK(hits[x] == 0);
    CHECK(std::memcmp(so.data(), want.data(), want.size()) == 0);
    for (size_t x = p.S * k; x < p.S * n; ++x) CHECK(so[x] == kFill);
  }
  // partial overlap: the object starts a few bytes into its shard buffer
  {
    const size_t shift = 1 + rng() % std::min<size_t>(7, p.S * n - 1);  // below n * S: they overlap
    std::vector<uint8_t> buf(p.S * n + shift, kFill), staged(p.S * k, 0x11), hits(p.S * n, 0);
    std::memcpy(buf.data() + shift, data.data(), len);
    SplitPlan q = p;
    split_prepare(q, n, buf.data() + shift, buf.data());
    CHECK(q.rows_from_data == 0);
    stage_rows(q, buf.data() + shift, buf.data(), split_tee(q, buf.data()), staged, hits);
    CHECK(staged == want);
    CHECK(std::memcmp(buf.data(), want.data(), want.size()) == 0);
  }
}

void check_decode(int k, size_t len, std::mt19937& rng) {
  const int n = k + kParity;
  const SplitPlan p = split_plan(k, len);
  const size_t S = p.S, kS = S * k;
  const std::vector<uint8_t> shards = random_bytes(S * n, rng);  // n shards back to back
  std::set<size_t> sizes = {0, 1, len, kS, kS + 1, kS + 100000};
  if (len > 1) sizes.insert(len - 1);
  for (size_t orig : sizes) {
    const size_t want = std::min(orig, kS);
    std::vector<uint8_t> out(std::max(orig, kS) + 64, kFill), hits(out.size(), 0);
    const Join j = decode_join(k, S, out.data(), orig);
    CHECK(j.out == out.data() && j.len == want && j.S == S && j.k == k);
    for (int i = 0; i < n; ++i)
      for (size_t col = 0; col < S; col += kCut) {
        const size_t w = std::min(kCut, S - col);
        const auto t = join_span(&j, i, col, w);
        if (!t.first) {
          CHECK(t.second == 0);
          continue;
        }
        CHECK(i < k && t.second >= 1 && t.second <= w);
        CHECK(t.first == out.data() + S * i + col);
        std::memcpy(t.first, &shards[S * i + col], t.second);
        for (size_t x = 0; x < t.second; ++x) ++hits[S * i + col + x];
      }
    for (size_t x = 0; x < out.size(); ++x) {
      CHECK(hits[x] == (x < want ? 1 : 0));
      CHECK(out[x] == (x < want ? shards[x] : kFill));
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(20240611u);
  size_t cases = 0;
  for (int k : {1, 3, 4, 10, 16, 255}) {
    const size_t K = static_cast<size_t>(k);
    const size_t large = (1u << 20) + rng() % (2u << 20);
    std::set<size_t> lens = {1, 2, K, K + 1, 16 * K - 1, 16 * K, 16 * K + 1, 8192 * K - 1, 8192 * K + 1, large};
    if (k > 1) lens.insert(K - 1);
    for (size_t len : lens) {
      g_k = k;
      g_len = len;
      check_encode(k, len, rng);
      check_decode(k, len, rng);
      ++cases;
    }
  }
  std::printf("%zu cases\ncodec_batch_test ok\n", cases);
  return 0;
}
