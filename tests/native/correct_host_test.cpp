// The correction rule of correct plans on the CPU, built with
// g++ -fsanitize=address,undefined by tests/test_native_correct.py. locate_correct is the
// function rs_apply_correct runs. For every pattern built from RS(10,4), (4,2), (3,2), (6,3),
// (1,3), (16,4), (10,8), (20,12) and (10,20) with everything present and under seeded masks, in
// every packing width the kernel instances use:
//  - every single error (every examined position, every e = 1..255): with r' >= 3 the verdict is
//    that shard, the position its place in T = valid then cmp, the value exactly e, and XORing
//    the value in at that position restores the codeword; with r' < 3 the verdict is
//    "unexplained" and neither position nor value is written;
//  - seeded columns with 2..r'-1 errors: unexplained, nothing written;
//  - a clean column is clean, and junk in shards that are not examined changes nothing;
//  - on every one of these cases with r' >= 3, and on seeded columns with r' or more errors, the
//    verdict is locate_classify's.
// A correct plan's tables are build_locate_tables(..., 1): nothing else is built here.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gf256.hpp"
#include "locate_tables.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// a * b in GF(2^8) mod 0x11D, no tables
uint8_t gmul(uint8_t a, uint8_t b) {
  unsigned r = 0, x = a;
  for (int i = 0; i < 8; ++i) {
    if ((b >> i) & 1u) r ^= x;
    x <<= 1;
    if (x & 0x100u) x ^= 0x11Du;
  }
  return static_cast<uint8_t>(r);
}

// The syndromes of one column, from the definition: stored cmp ^ G . valid.
std::vector<uint8_t> syndromes(const std::vector<uint8_t>& col, const std::vector<int>& valid,
                               const std::vector<int>& cmp, const Mat& G, int rows) {
  std::vector<uint8_t> s(static_cast<size_t>(rows));
  for (int x = 0; x < rows; ++x) {
    uint8_t v = col[static_cast<size_t>(cmp[static_cast<size_t>(x)])];
    for (size_t j = 0; j < valid.size(); ++j)
      v ^= gmul(G.at(x, static_cast<int>(j)), col[static_cast<size_t>(valid[j])]);
    s[static_cast<size_t>(x)] = v;
  }
  return s;
}

constexpr uint32_t kUnset = 0xdeadbeefu;
struct Fix {
  uint32_t verdict, pos, value;
  bool operator==(const Fix& o) const { return verdict == o.verdict && pos == o.pos && value == o.value; }
};

template <int NW>
Fix correct(const std::vector<uint8_t>& s, int rows, int k, const uint8_t* gf, const uint8_t* pt) {
  uint32_t w[NW] = {0};
  // junk at and past `rows` must not be read
  for (int x = 0; x < NW * 4; ++x)
    w[x >> 2] |= static_cast<uint32_t>(x < rows ? s[static_cast<size_t>(x)] : 0xA5u) << (8 * (x & 3));
  Fix f{0, kUnset, kUnset};
  f.verdict = locate_correct(w, rows, k, gf, pt, f.pos, f.value);
  // the verdict is locate_classify's wherever a column may be corrected at all
  if (rows >= 3) CHECK(f.verdict == locate_classify(w, rows, k, gf, pt));
  // position and value are written with a shard verdict, and only then
  if (f.verdict >= 256u) CHECK(f.pos == kUnset && f.value == kUnset);
  return f;
}

Fix correct_all(const std::vector<uint8_t>& s, int rows, int k, const uint8_t* gf, const uint8_t* pt) {
  const Fix f = correct<4>(s, rows, k, gf, pt);
  if (rows <= 8) CHECK(correct<2>(s, rows, k, gf, pt) == f);
  if (rows <= 4) CHECK(correct<1>(s, rows, k, gf, pt) == f);
  return f;
}

long g_singles = 0, g_gated = 0, g_multis = 0, g_heavy = 0;

void check_pattern(int k, int m, const LocateTables& t, size_t p, std::mt19937& rng) {
  const int n = k + m;
  const MixedPattern& pt = t.ragged.mixed.patterns[p];
  const uint8_t* blk = &t.loc[p * t.stride];
  const uint8_t* gf = t.gf.data();
  const std::vector<uint8_t> none(static_cast<size_t>(n), 0);
  DecodePlan dp;
  CHECK(decode_plan(k, m, pt.mask.data(), none.data(), dp));
  const int rows = static_cast<int>(t.rows(p));
  if (rows == 0) return;
  // a codeword column: E . data
  Mat E;
  CHECK(encode_matrix(k, m, E));
  std::vector<uint8_t> data(static_cast<size_t>(k)), col(static_cast<size_t>(n), 0);
  for (auto& d : data) d = static_cast<uint8_t>(rng());
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < k; ++j) col[static_cast<size_t>(i)] ^= gmul(E.at(i, j), data[static_cast<size_t>(j)]);
  std::vector<int> cmp(dp.check.begin(), dp.check.begin() + rows);
  std::vector<int> T(dp.valid);  // position -> shard
  T.insert(T.end(), cmp.begin(), cmp.end());
  auto run = [&](const std::vector<uint8_t>& c) {
    return correct_all(syndromes(c, dp.valid, cmp, dp.rows, rows), rows, k, gf, blk);
  };
  CHECK(run(col).verdict == kLocateClean);
  // every single error
  for (size_t at = 0; at < T.size(); ++at)
    for (int e = 1; e < 256; ++e) {
      std::vector<uint8_t> bad(col);
      bad[static_cast<size_t>(T[at])] ^= static_cast<uint8_t>(e);
      const Fix f = run(bad);
      if (rows < 3) {
        CHECK(f.verdict == kLocateUnexplained);
        ++g_gated;
        continue;
      }
      CHECK(f.verdict == static_cast<uint32_t>(T[at]) && f.pos == at && f.value == static_cast<uint32_t>(e));
      bad[static_cast<size_t>(T[f.pos])] ^= static_cast<uint8_t>(f.value);
      CHECK(bad == col);
      ++g_singles;
    }
  // junk in shards that are not examined changes nothing
  {
    std::vector<uint8_t> bad(col);
    for (int i = 0; i < n; ++i) {
      bool ex = false;
      for (int s : T) ex |= s == i;
      if (!ex) bad[static_cast<size_t>(i)] ^= 0x5a;
    }
    CHECK(run(bad).verdict == kLocateClean);
  }
  // 2 .. rows-1 errors: unexplained, nothing written; rows or more: whatever locate_classify says
  for (int c = 0; rows >= 3 && c < 400; ++c) {
    const bool heavy = c >= 300;
    const int nerr = heavy ? rows + static_cast<int>(rng() % 2u)
                           : 2 + static_cast<int>(rng() % static_cast<unsigned>(rows - 2));
    std::vector<int> pos(T);
    std::vector<uint8_t> bad(col);
    for (int q = 0; q < nerr && q < static_cast<int>(pos.size()); ++q) {
      const size_t at = static_cast<size_t>(q) + rng() % (pos.size() - static_cast<size_t>(q));
      std::swap(pos[static_cast<size_t>(q)], pos[at]);
      bad[static_cast<size_t>(pos[static_cast<size_t>(q)])] ^= static_cast<uint8_t>(1 + rng() % 255);
    }
    const Fix f = run(bad);
    if (heavy) {
      ++g_heavy;
    } else {
      CHECK(f.verdict == kLocateUnexplained);
      ++g_multis;
    }
  }
}

void profile(int k, int m, std::mt19937& rng) {
  const int n = k + m;
  // stripe 0 everything present, then seeded masks with k .. n shards present
  const int batch = 6;
  std::vector<uint8_t> pres(static_cast<size_t>(batch) * n, 1);
  std::vector<size_t> sizes(static_cast<size_t>(batch));
  for (int b = 0; b < batch; ++b) sizes[static_cast<size_t>(b)] = 1 + rng() % 40000;
  for (int b = 1; b < batch; ++b) {
    // b = 1: one missing, b = 2: r' = 2 where m allows it, then seeded
    const int drop = b == 1 ? 1 : b == 2 ? std::max(0, m - 2) : static_cast<int>(rng() % static_cast<unsigned>(m));
    for (int d = 0; d < drop;) {
      const size_t i = rng() % static_cast<unsigned>(n);
      if (!pres[static_cast<size_t>(b) * n + i]) continue;
      pres[static_cast<size_t>(b) * n + i] = 0;
      ++d;
    }
  }
  LocateTables t;
  CHECK(build_locate_tables(k, m, batch, sizes.data(), pres.data(), t, 1) == TableError::kOk);
  CHECK(t.gf.size() == kLocGfBytes && t.stride == locate_stride(k));
  for (size_t p = 0; p < t.ragged.mixed.patterns.size(); ++p) check_pattern(k, m, t, p, rng);
}

}  // namespace

int main() {
  std::mt19937 rng(20261021);
  const int profiles[][2] = {{10, 4}, {4, 2}, {3, 2}, {6, 3}, {1, 3}, {16, 4}, {10, 8}, {20, 12}, {10, 20}};
  for (const auto& pr : profiles) profile(pr[0], pr[1], rng);
  CHECK(g_singles > 0 && g_gated > 0 && g_multis > 0 && g_heavy > 0);
  std::printf("singles %ld gated %ld multis %ld heavy %ld\ncorrect_host_test ok\n", g_singles, g_gated, g_multis,
              g_heavy);
  return 0;
}
