// Host-side tables of required device plans on the CPU, built with
// g++ -fsanitize=address,undefined by tests/test_native_required.py:
//  - decode_plan with a wanted set is the matching subset of the full plan's rows, for RS(4,2)
//    over every (mask, wanted) pair and for RS(10,4) over seeded pairs;
//  - build_mixed_tables' arenas for a wanted set, applied with a scalar GF(2^8) lookup to the shards
//    a pattern reads, give the bytes of the shards its rows name (those of a consistent stripe:
//    what a full reconstruct writes) for rows below nrows, and are zero past nrows;
//  - patterns are deduplicated on the (mask, wanted) pair;
//  - each launch group's tile map holds exactly the stripes with a row in the group (RS(3,20):
//    16 + 4 rows); stripes with no row are in no map, a batch of such stripes has no group;
//  - the index of an unwanted missing shard is in no pattern's `valid` or `rows`: its pointer
//    reaches no in_tab or out_tab;
//  - the host calls' admission with a wanted set (host_path.hpp admit_stripe) and the classes
//    and segments their ragged runs are cut into (ragged_chunks.hpp).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "gf256.hpp"
#include "host_path.hpp"
#include "mixed_tables.hpp"
#include "ragged_chunks.hpp"
#include "ragged_tables.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

void check_decode_plan(int k, int m, const uint8_t* pres, const uint8_t* want) {
  const int n = k + m;
  DecodePlan full, some;
  CHECK(decode_plan(k, m, pres, full));
  CHECK(decode_plan(k, m, pres, want, some));
  CHECK(some.valid == full.valid);
  CHECK(some.check == full.check);
  std::vector<int> missing;
  std::vector<int> from;  // row of `full` behind each row of `some`
  for (size_t r = 0; r < full.missing.size(); ++r)
    if (want[full.missing[r]]) {
      missing.push_back(full.missing[r]);
      from.push_back(static_cast<int>(r));
    }
  for (size_t r = 0; r < full.check.size(); ++r) from.push_back(static_cast<int>(full.missing.size() + r));
  CHECK(some.missing == missing);
  for (int i : some.missing) CHECK(i >= 0 && i < n && !pres[i] && want[i]);
  CHECK(some.rows.rows == static_cast<int>(from.size()) && some.rows.cols == k);
  for (size_t r = 0; r < from.size(); ++r)
    for (int i = 0; i < k; ++i) CHECK(some.rows.at(static_cast<int>(r), i) == full.rows.at(from[r], i));
  // a null wanted set and an all-ones one are the full plan
  DecodePlan all;
  std::vector<uint8_t> ones(static_cast<size_t>(n), 1);
  CHECK(decode_plan(k, m, pres, ones.data(), all));
  CHECK(all.missing == full.missing && all.check == full.check && all.rows.v == full.rows.v);
  CHECK(decode_plan(k, m, pres, nullptr, all));
  CHECK(all.missing == full.missing && all.rows.v == full.rows.v);
}

void decode_plans() {
  int pairs = 0;
  {  // RS(4,2): every mask with at least k present, every wanted set
    const int k = 4, m = 2, n = 6;
    for (unsigned pm = 0; pm < (1u << n); ++pm) {
      if (__builtin_popcount(pm) < k) continue;
      for (unsigned wm = 0; wm < (1u << n); ++wm) {
        uint8_t pres[6], want[6];
        for (int i = 0; i < n; ++i) {
          pres[i] = (pm >> i) & 1u;
          want[i] = (wm >> i) & 1u;
        }
        check_decode_plan(k, m, pres, want);
        ++pairs;
      }
    }
  }
  std::mt19937 rng(1234);
  for (int c = 0; c < 200; ++c) {
    const int k = 10, m = 4, n = 14;
    uint8_t pres[14], want[14];
    for (int i = 0; i < n; ++i) {
      pres[i] = 1;
      want[i] = rng() & 1u;
    }
    for (int l = static_cast<int>(rng() % 5u); l > 0;) {
      const int i = static_cast<int>(rng() % 14u);
      if (pres[i]) {
        pres[i] = 0;
        --l;
      }
    }
    check_decode_plan(k, m, pres, want);
    ++pairs;
  }
  std::printf("decode_plan with a wanted set: %d pairs ok\n", pairs);
}

// A consistent stripe: k random data shards and their parity by the encoding matrix.
std::vector<std::vector<uint8_t>> make_stripe(int k, int m, size_t S, std::mt19937& rng) {
  Mat E;
  CHECK(encode_matrix(k, m, E));
  std::vector<std::vector<uint8_t>> st(static_cast<size_t>(k + m), std::vector<uint8_t>(S));
  for (int i = 0; i < k; ++i)
    for (size_t x = 0; x < S; ++x) st[i][x] = static_cast<uint8_t>(rng());
  for (int j = k; j < k + m; ++j)
    for (size_t x = 0; x < S; ++x) {
      uint8_t v = 0;
      for (int i = 0; i < k; ++i) v ^= gf().mul[E.at(j, i)][st[i][x]];
      st[j][x] = v;
    }
  return st;
}

struct Batch {
  int k, m, batch;
  std::vector<uint8_t> pres, want;
  std::vector<size_t> sizes;
};

// Seeded masks with 0..m lost and a seeded wanted set; stripe 0 has exactly k present and
// wants nothing (r = 0), stripe 1 loses m and wants all of them, stripe 2 repeats stripe 1's
// mask with another wanted set, stripe 3 repeats stripe 1 (one pattern).
Batch make_batch(int k, int m, int batch, unsigned seed) {
  const int n = k + m;
  std::mt19937 rng(seed);
  Batch b{k, m, batch, std::vector<uint8_t>(static_cast<size_t>(batch) * n, 1),
          std::vector<uint8_t>(static_cast<size_t>(batch) * n, 0), std::vector<size_t>(batch)};
  for (int s = 0; s < batch; ++s) {
    b.sizes[s] = 1 + rng() % 30000;
    uint8_t* p = &b.pres[static_cast<size_t>(s) * n];
    uint8_t* w = &b.want[static_cast<size_t>(s) * n];
    for (int l = s < 4 ? m : static_cast<int>(rng() % static_cast<unsigned>(m + 1)); l > 0;) {
      const int i = s < 4 ? l : static_cast<int>(rng() % static_cast<unsigned>(n));  // 1..m for s < 4
      if (p[i]) {
        p[i] = 0;
        --l;
      }
    }
    for (int i = 0; i < n; ++i) w[i] = s == 0 ? p[i] : s == 1 || s == 3 ? 1 : s == 2 ? (i & 1) : rng() & 1u;
  }
  return b;
}

int rows_of(const MixedTables& t, int s) { return static_cast<int>(t.patterns[t.pat[s]].rows.size()); }

void check_required(int k, int m, int batch, unsigned seed) {
  const int n = k + m;
  const Batch b = make_batch(k, m, batch, seed);
  RaggedTables rq;
  CHECK(build_ragged_tables(k, m, batch, b.sizes.data(), b.pres.data(), b.want.data(), rq) ==
        TableError::kOk);
  const MixedTables& t = rq.mixed;
  CHECK(t.k == k && t.m == m && t.batch == batch && static_cast<int>(t.pat.size()) == batch);

  // patterns: one per distinct (mask, wanted missing) pair, in order of first appearance
  std::vector<std::pair<std::vector<uint8_t>, std::vector<uint8_t>>> seen;
  for (int s = 0; s < batch; ++s) {
    std::vector<uint8_t> mask(b.pres.begin() + s * n, b.pres.begin() + (s + 1) * n), wm(n, 0);
    for (int i = 0; i < n; ++i) wm[i] = !mask[i] && b.want[static_cast<size_t>(s) * n + i];
    size_t at = 0;
    while (at < seen.size() && seen[at] != std::make_pair(mask, wm)) ++at;
    if (at == seen.size()) seen.emplace_back(mask, wm);
    CHECK(t.pat[s] == at);
  }
  CHECK(seen.size() == static_cast<size_t>(t.P()));
  CHECK(t.pat[1] == t.pat[3] && t.pat[1] != t.pat[2]);
  CHECK(t.patterns[t.pat[1]].mask == t.patterns[t.pat[2]].mask);

  uint64_t bytes = 0;
  int max_rows = 0;
  for (int p = 0; p < t.P(); ++p) {
    const MixedPattern& pt = t.patterns[p];
    CHECK(pt.mask == seen[p].first);
    DecodePlan dp;
    CHECK(decode_plan(k, m, pt.mask.data(), seen[p].second.data(), dp));
    CHECK(pt.valid == dp.valid && pt.missing == static_cast<int>(dp.missing.size()));
    std::vector<int> rows = dp.missing;
    rows.insert(rows.end(), dp.check.begin(), dp.check.end());
    CHECK(pt.rows == rows);
    CHECK(static_cast<int>(rows.size()) <= m);
    max_rows = std::max(max_rows, static_cast<int>(rows.size()));
    // the NULL contract: an unwanted missing shard is named nowhere
    for (int i = 0; i < n; ++i) {
      if (pt.mask[i] || seen[p].second[i]) continue;
      CHECK(std::find(pt.valid.begin(), pt.valid.end(), i) == pt.valid.end());
      CHECK(std::find(pt.rows.begin(), pt.rows.end(), i) == pt.rows.end());
    }
    for (int i : pt.valid) CHECK(pt.mask[i]);
    for (int r = 0; r < static_cast<int>(rows.size()); ++r)
      CHECK(r < pt.missing ? seen[p].second[rows[r]] != 0 : pt.mask[rows[r]] != 0);
  }
  CHECK(rows_of(t, 0) == 0 && rows_of(t, 1) == m);
  CHECK(t.rows == max_rows);
  bool uniform = true;
  for (const MixedPattern& pt : t.patterns) uniform &= static_cast<int>(pt.rows.size()) == max_rows;
  CHECK(t.uniform_rows == uniform && !uniform && !mixed_rows_are(t, max_rows));
  CHECK(static_cast<int>(t.groups.size()) == (max_rows + kMixedRowsPerLaunch - 1) / kMixedRowsPerLaunch);
  CHECK(rq.maps.size() == t.groups.size());
  for (int s = 0; s < batch; ++s)
    if (rows_of(t, s)) bytes += b.sizes[s] * static_cast<uint64_t>(k + rows_of(t, s));
  CHECK(rq.bytes == bytes);

  std::mt19937 rng(seed + 1);
  for (size_t gi = 0; gi < t.groups.size(); ++gi) {
    const MixedGroup& g = t.groups[gi];
    const int W = nibble_width(g.R);
    CHECK(g.row0 == static_cast<int>(gi) * kMixedRowsPerLaunch);
    CHECK(g.R == std::min(kMixedRowsPerLaunch, max_rows - g.row0));
    CHECK(g.tab_stride == static_cast<size_t>(k) * 32u * W);
    CHECK(g.arena.size() == g.tab_stride * t.P() && g.nrows.size() == static_cast<size_t>(t.P()));
    for (int p = 0; p < t.P(); ++p) {
      const MixedPattern& pt = t.patterns[p];
      const int nr = std::max(0, std::min(g.R, static_cast<int>(pt.rows.size()) - g.row0));
      CHECK(g.nrows[p] == static_cast<uint32_t>(nr));
      uint32_t vm = 0;
      for (int r = 0; r < nr; ++r)
        if (g.row0 + r >= pt.missing) vm |= 1u << r;
      CHECK(g.vmask[p] == vm);
      // the tables applied to a consistent stripe give the shards the rows name
      const size_t S = 37;
      const auto st = make_stripe(k, m, S, rng);
      const uint8_t* tab = &g.arena[p * g.tab_stride];
      for (size_t x = 0; x < S; ++x) {
        uint8_t acc[16] = {0};
        for (int i = 0; i < k; ++i) {
          const uint8_t v = st[pt.valid[i]][x];
          const uint8_t* ti = tab + static_cast<size_t>(i) * 32u * W;
          for (int c = 0; c < W; ++c) acc[c] ^= ti[(v & 15u) * W + c] ^ ti[(16u + (v >> 4)) * W + c];
        }
        for (int r = 0; r < nr; ++r) CHECK(acc[r] == st[pt.rows[g.row0 + r]][x]);
      }
      // columns at and past nrows are zero
      for (int i = 0; i < k; ++i)
        for (int e = 0; e < 32; ++e)
          for (int c = nr; c < W; ++c) CHECK(tab[(static_cast<size_t>(i) * 32u + e) * W + c] == 0);
    }
    // the group's tile map: exactly the stripes with a row in the group, in order
    const TileMap& gm = rq.maps[gi];
    CHECK(gm.tile0.size() == static_cast<size_t>(batch) + 1);
    uint32_t at = 0;
    int stripes = 0;
    bool tail = false;
    for (int s = 0; s < batch; ++s) {
      CHECK(gm.tile0[s] == at);
      if (rows_of(t, s) <= g.row0) continue;
      for (uint64_t i = 0; i < ragged_tiles(b.sizes[s]); ++i) CHECK(gm.tile_stripe.at(at + i) == static_cast<uint32_t>(s));
      at += static_cast<uint32_t>(ragged_tiles(b.sizes[s]));
      ++stripes;
      tail |= b.sizes[s] % 16 != 0;
    }
    CHECK(gm.tile0[batch] == at && gm.ntiles == at && gm.tile_stripe.size() == at);
    CHECK(gm.stripes == stripes && stripes > 0 && gm.any_tail == tail);
    for (uint32_t s : gm.tile_stripe) CHECK(g.nrows[t.pat[s]] >= 1);
    std::printf("RS(%d,%d) group %zu: R %d, %d of %d stripes, %u tiles ok\n", k, m, gi, g.R, stripes,
                batch, gm.ntiles);
  }
}

void two_groups() {
  // RS(3,20): 16 + 4 rows; stripes with at most 16 rows are in the first group's map alone
  const int k = 3, m = 20, n = 23, batch = 6;
  const int lost[batch] = {20, 20, 20, 4, 20, 1};    // shards 1..lost are missing
  const int wanted[batch] = {20, 16, 17, 0, 0, 1};    // of which the first `wanted` are wanted
  const int rows[batch] = {20, 16, 17, 16, 0, 20};    // w + c, c = 20 - lost
  std::vector<uint8_t> pres(batch * n, 1), want(batch * n, 0);
  std::vector<size_t> sizes = {8193, 5, 40000, 16, 9000, 8192};
  for (int s = 0; s < batch; ++s)
    for (int i = 1; i <= lost[s]; ++i) {
      pres[s * n + i] = 0;
      want[s * n + i] = i <= wanted[s];
    }
  RaggedTables rq;
  CHECK(build_ragged_tables(k, m, batch, sizes.data(), pres.data(), want.data(), rq) == TableError::kOk);
  for (int s = 0; s < batch; ++s) CHECK(rows_of(rq.mixed, s) == rows[s]);
  CHECK(rq.mixed.groups.size() == 2 && rq.mixed.groups[0].R == 16 && rq.mixed.groups[1].R == 4);
  CHECK(rq.maps[0].stripes == 5 && rq.maps[1].stripes == 3);
  const std::set<uint32_t> second(rq.maps[1].tile_stripe.begin(), rq.maps[1].tile_stripe.end());
  CHECK(second == (std::set<uint32_t>{0, 2, 5}));
  const std::set<uint32_t> first(rq.maps[0].tile_stripe.begin(), rq.maps[0].tile_stripe.end());
  CHECK(first == (std::set<uint32_t>{0, 1, 2, 3, 5}));
  CHECK(rq.mixed.groups[1].nrows[rq.mixed.pat[2]] == 1 && rq.mixed.groups[1].nrows[rq.mixed.pat[1]] == 0);
  CHECK(rq.maps[1].ntiles == 1 + 5 + 1);
  std::printf("RS(3,20): 16 + 4 rows, the second group's map skips the short patterns ok\n");
}

void no_rows_and_errors() {
  const int k = 4, m = 2, n = 6;
  // only stripes with exactly k present and nothing wanted: no group, no map, no bytes
  std::vector<uint8_t> pres = {1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 1};
  std::vector<uint8_t> want = {1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0};
  std::vector<size_t> sizes = {100, 9000};
  RaggedTables rq;
  CHECK(build_ragged_tables(k, m, 2, sizes.data(), pres.data(), want.data(), rq) == TableError::kOk);
  CHECK(rq.mixed.groups.empty() && rq.maps.empty() && rq.bytes == 0 && rq.mixed.rows == 0);
  CHECK(rq.mixed.P() == 2 && rq.mixed.patterns[0].rows.empty());
  CHECK(!required_all_wanted(n, 2, pres.data(), want.data()));
  CHECK(!required_pairs_equal(n, 2, pres.data(), want.data()));
  if (sizeof(size_t) >= 8) {
    // the tile and byte limits count the stripes with a row alone; too few shards comes first
    sizes[1] = ~static_cast<size_t>(0);
    CHECK(build_ragged_tables(k, m, 2, sizes.data(), pres.data(), want.data(), rq) == TableError::kOk);
    CHECK(rq.bytes == 0 && rq.maps.empty());
    want[6] = 1;  // stripe 1 wants its shard 0: one row over 2^64 - 1 bytes
    CHECK(build_ragged_tables(k, m, 2, sizes.data(), pres.data(), want.data(), rq) == TableError::kTooManyTiles);
    sizes[1] = static_cast<size_t>(1) << 45;  // no byte overflow, 2^32 tiles
    CHECK(build_ragged_tables(k, m, 2, sizes.data(), pres.data(), want.data(), rq) == TableError::kTooManyTiles);
    pres[2] = 0;
    CHECK(build_ragged_tables(k, m, 2, sizes.data(), pres.data(), want.data(), rq) == TableError::kTooFewShards);
    pres[2] = 1;
    want[6] = 0;
    sizes[1] = 9000;
  }
  // errors: a zero size, k - 1 present shards
  sizes[1] = 0;
  CHECK(build_ragged_tables(k, m, 2, sizes.data(), pres.data(), want.data(), rq) == TableError::kNoData);
  sizes[1] = 5;
  pres[2] = 0;
  CHECK(build_ragged_tables(k, m, 2, sizes.data(), pres.data(), want.data(), rq) == TableError::kTooFewShards);
  // the routing predicates: flags on present shards count for nothing
  std::vector<uint8_t> p2 = {1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1};
  std::vector<uint8_t> w2 = {0, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 1};
  CHECK(required_all_wanted(n, 2, p2.data(), w2.data()));
  CHECK(required_all_wanted(n, 2, p2.data(), nullptr));
  CHECK(required_pairs_equal(n, 2, p2.data(), w2.data()));
  w2[7] = 0;
  CHECK(!required_all_wanted(n, 2, p2.data(), w2.data()));
  CHECK(!required_pairs_equal(n, 2, p2.data(), w2.data()));
  w2[1] = 0;
  CHECK(required_pairs_equal(n, 2, p2.data(), w2.data()));
  std::printf("no rows, errors and routing predicates ok\n");
}

void host_admission_and_classes() {
  const int k = 4, m = 2, n = 6;
  uint8_t buf[8] = {0};
  auto admit = [&](std::vector<size_t> lens, std::vector<uint8_t> want, std::vector<int> null, bool verify,
                   std::vector<uint8_t>* flags) {
    std::vector<const uint8_t*> sh(n, buf);
    for (int i : null) sh[i] = nullptr;
    flags->assign(n, 9);
    return admit_stripe(n, k, sh.data(), lens.data(), want.data(), verify, flags->data());
  };
  std::vector<uint8_t> f;
  // one wanted, one unwanted (NULL) missing shard
  StripeAdmission a = admit({8, 0, 8, 8, 8, 0}, {0, 1, 1, 0, 0, 0}, {5}, false, &f);
  CHECK(a.run && a.status == RS_OK && a.S == 8);
  CHECK((f == std::vector<uint8_t>{kShardPresent, kShardWanted, kShardPresent, kShardPresent, kShardPresent,
                                   kShardUnwanted}));
  // a NULL wanted shard, a NULL present shard
  CHECK(admit({8, 0, 8, 8, 8, 0}, {0, 1, 0, 0, 0, 0}, {1}, false, &f).status == RS_E_ARG);
  CHECK(admit({8, 0, 8, 8, 8, 0}, {0, 1, 0, 0, 0, 0}, {2}, false, &f).status == RS_E_ARG);
  // nothing wanted: without verify nothing to do (whatever is NULL), with verify the compared row runs
  a = admit({8, 0, 8, 8, 8, 8}, {1, 0, 1, 0, 0, 0}, {1}, false, &f);
  CHECK(!a.run && a.status == RS_OK);
  a = admit({8, 0, 8, 8, 8, 8}, {1, 0, 1, 0, 0, 0}, {1}, true, &f);
  CHECK(a.run && a.status == RS_OK && f[1] == kShardUnwanted);
  // exactly k present, nothing wanted, verify: no row, but admitted (flags and S written)
  a = admit({8, 0, 8, 8, 8, 0}, {1, 0, 0, 0, 0, 0}, {1, 5}, true, &f);
  CHECK(!a.run && a.status == RS_OK && a.S == 8 && f[1] == kShardUnwanted && f[0] == kShardPresent);
  // upstream's order: sizes, then too few shards, whatever is wanted
  CHECK(admit({8, 0, 7, 8, 8, 0}, {0, 1, 0, 0, 0, 0}, {}, true, &f).status == RS_E_SHARD_SIZE);
  CHECK(admit({8, 0, 0, 8, 8, 0}, {0, 0, 0, 0, 0, 0}, {}, true, &f).status == RS_E_TOO_FEW_SHARDS);
  CHECK(admit({0, 0, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 1}, {}, true, &f).status == RS_E_NO_DATA);

  // classes by row count r = w + (verify: present - k); r = 0 in no class
  const uint8_t P = kShardPresent, W = kShardWanted, U = kShardUnwanted;
  const std::vector<uint8_t> flags = {
      P, W, P, P, P, U,  // w 1, c 0
      P, U, P, P, P, U,  // w 0, c 0
      P, W, P, P, P, P,  // w 1, c 1
      P, P, P, P, P, P,  // w 0, c 2
      W, W, P, P, P, P,  // w 2, c 0
      P, U, P, P, P, P,  // w 0, c 1
  };
  auto cls = ragged_classes(n, k, 6, flags.data(), true);
  CHECK(cls.size() == 2 && cls[0].rows == 1 && cls[1].rows == 2);
  CHECK((cls[0].stripes == std::vector<int>{0, 5}) && (cls[1].stripes == std::vector<int>{2, 3, 4}));
  cls = ragged_classes(n, k, 6, flags.data(), false);
  CHECK(cls.size() == 2 && cls[0].rows == 1 && cls[1].rows == 2);
  CHECK((cls[0].stripes == std::vector<int>{0, 2}) && (cls[1].stripes == std::vector<int>{4}));
  CHECK(ragged_classes(n, k, 1, flags.data() + n, true).empty());
  // segments: one mask with two wanted sets is two patterns
  const std::vector<uint8_t> two = {P, W, P, P, P, U, P, U, P, P, P, W, P, W, P, P, P, U};
  const size_t per = pattern_arena_bytes(k, 1);
  auto segs = ragged_segments(k, n, 1, {0, 1, 2}, two.data(), per);
  CHECK(segs.size() == 3);
  segs = ragged_segments(k, n, 1, {0, 2, 1}, two.data(), per);
  CHECK(segs.size() == 2 && segs[0] == std::make_pair(size_t(0), size_t(2)));
  segs = ragged_segments(k, n, 1, {0, 1, 2}, two.data(), 2 * per);
  CHECK(segs.size() == 1);
  // every pattern of a class has the class's rows: the tables the ragged kernels expect
  for (bool verify : {true, false})
    for (const RaggedClass& c : ragged_classes(n, k, 6, flags.data(), verify)) {
      std::vector<uint8_t> pres, want;
      for (int b : c.stripes)
        for (int i = 0; i < n; ++i) {
          pres.push_back(flags[b * n + i] == P);
          want.push_back(flags[b * n + i] == W);
        }
      MixedTables t;
      CHECK(build_mixed_tables(k, m, static_cast<int>(c.stripes.size()), pres.data(), want.data(), t, verify) ==
            TableError::kOk);
      CHECK(t.rows == c.rows && t.uniform_rows && mixed_rows_are(t, c.rows) && !mixed_rows_are(t, c.rows + 1));
      for (const MixedPattern& pt : t.patterns) CHECK(static_cast<int>(pt.rows.size()) == c.rows);
      for (const MixedGroup& g : t.groups)
        for (uint32_t nr : g.nrows) CHECK(static_cast<int>(nr) == g.R);
    }
  std::printf("host admission, classes and segments ok\n");
}

}  // namespace

int main() {
  decode_plans();
  check_required(10, 4, 40, 7);
  check_required(6, 8, 24, 8);
  check_required(5, 12, 24, 9);
  check_required(3, 20, 30, 10);
  check_required(4, 2, 12, 11);
  two_groups();
  no_rows_and_errors();
  host_admission_and_classes();
  std::printf("required_host_test ok\n");
  return 0;
}
