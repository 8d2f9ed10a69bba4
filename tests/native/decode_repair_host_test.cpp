// Host-side tables of decode-repair device plans and the rule the kernel runs,
// on the CPU, built with g++ -fsanitize=address,undefined by tests/test_native_decode_repair.py:
//  - a pattern's row list is its compared indices ascending, then its wanted indices ascending;
//    cmask is the low r' bits; one launch group; the arena against a bit-by-bit GF(2^8) multiply;
//  - the locate block: the ratio table over all k expected positions from check rows 0 and 1, the
//    position map V then the compared shards, G by column over all rows, wanted rows included,
//    against decode_plan's rows and the bit-by-bit multiply; the byte counts; the fix slots;
//  - repair_mul_word against the bit-by-bit multiply, every g and every byte in every lane;
//  - every refusal in its order, the fix placement and the 17-row limit included;
//  - a scalar model of the whole rule, merge and store: every single error at every expected and
//    compared position with every value repaired exactly, 2..r'-1 errors left unexplained with
//    the wanted bytes as computed, r' = 1 and 2 repairing nothing.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "decode_repair_tables.hpp"
#include "gf256.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// bit-by-bit multiply mod 0x11D: independent of gf256.hpp's log / exp tables
uint8_t slow_mul(uint8_t a, uint8_t b) {
  unsigned r = 0, x = a;
  for (int bit = 0; bit < 8; ++bit) {
    if ((b >> bit) & 1u) r ^= x;
    x <<= 1;
    if (x & 0x100u) x ^= 0x11Du;
  }
  return static_cast<uint8_t>(r);
}

struct Stripe {
  std::vector<int> expect, wanted, compared, delivered, fix;
  size_t size;
};

struct Flags {
  std::vector<uint8_t> expect, in, dst, chk, fix;
  std::vector<size_t> sizes;
};

Flags flags_of(int n, const std::vector<Stripe>& st) {
  Flags f;
  f.expect.assign(st.size() * n, 0);
  f.in = f.dst = f.chk = f.fix = f.expect;
  for (size_t b = 0; b < st.size(); ++b) {
    for (int i : st[b].expect) f.expect[b * n + i] = static_cast<uint8_t>(1 + (i % 3));  // any nonzero value
    for (int i : st[b].delivered) f.in[b * n + i] = 1;
    for (int i : st[b].wanted) f.dst[b * n + i] = 7;
    for (int i : st[b].compared) f.chk[b * n + i] = 9;
    for (int i : st[b].fix) f.fix[b * n + i] = 3;
    f.sizes.push_back(st[b].size);
  }
  return f;
}

std::vector<int> sorted(std::vector<int> v) {
  std::sort(v.begin(), v.end());
  return v;
}

DecodeRepairError build(int k, int m, const std::vector<Stripe>& st, DecodeRepairTables& t) {
  const Flags f = flags_of(k + m, st);
  return build_decode_repair_tables(k, m, static_cast<int>(st.size()), f.sizes.data(), f.expect.data(),
                                    f.in.data(), f.dst.data(), f.chk.data(), f.fix.data(), t);
}

// G = E[rows] . inv(E[V]) from decode_plan, independent of the tables under test: row of shard i
std::vector<uint8_t> g_row(int k, int m, const std::vector<int>& expect, int shard) {
  std::vector<uint8_t> present(static_cast<size_t>(k + m), 0);
  for (int i : expect) present[static_cast<size_t>(i)] = 1;
  DecodePlan dp;
  CHECK(decode_plan(k, m, present.data(), dp));
  const int row = static_cast<int>(std::find(dp.missing.begin(), dp.missing.end(), shard) - dp.missing.begin());
  CHECK(row < m);
  std::vector<uint8_t> g(static_cast<size_t>(k));
  for (int j = 0; j < k; ++j) g[static_cast<size_t>(j)] = dp.rows.at(row, j);
  return g;
}

void check_tables(int k, int m, const std::vector<Stripe>& st, const DecodeRepairTables& t) {
  const int batch = static_cast<int>(st.size());
  CHECK(t.stride == locate_stride(k) && t.gf.size() == kLocGfBytes);
  for (int a = 1; a < 256; ++a) CHECK(slow_mul(2, t.gf[256 + t.gf[static_cast<size_t>(a)]]) == slow_mul(2, static_cast<uint8_t>(a)));
  CHECK(t.nchk.size() == t.c.patterns.size() && t.loc.size() == t.c.patterns.size() * t.stride);
  uint64_t merge = 0, store = 0;
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    const Stripe& s = st[static_cast<size_t>(b)];
    const bool has = (!s.delivered.empty() && (!s.wanted.empty() || !s.compared.empty())) || !s.compared.empty();
    CHECK(t.c.has[static_cast<size_t>(b)] == has);
    if (!has) continue;
    any = true;
    merge += s.size * (s.delivered.size() + 2 * s.wanted.size() + s.compared.size());
    store += s.size * (s.delivered.size() + s.wanted.size());
    const uint32_t p = t.c.pat[static_cast<size_t>(b)];
    const DecodeCheckPattern& pt = t.c.patterns[p];
    std::vector<int> rows = sorted(s.compared);
    const std::vector<int> w = sorted(s.wanted);
    rows.insert(rows.end(), w.begin(), w.end());
    CHECK(pt.rows == rows && pt.expect == sorted(s.expect) && pt.delivered == sorted(s.delivered));
    CHECK(t.nchk[p] == s.compared.size() && t.c.nrows[p] == rows.size());
    for (size_t r = 0; r < rows.size(); ++r) CHECK((pt.check[r] != 0) == (r < s.compared.size()));
  }
  CHECK(t.c.bytes[2] == merge && t.c.bytes[3] == store);
  CHECK(t.c.groups.size() == (any ? 1u : 0u));
  if (!any) return;
  const DecodeCheckGroup& g = t.c.groups[0];
  CHECK(g.row0 == 0 && g.R == t.c.rmax && g.R <= kRepairRows);
  const int W = nibble_width(g.R);
  const size_t per = 32u * static_cast<size_t>(W);
  for (size_t p = 0; p < t.c.patterns.size(); ++p) {
    const DecodeCheckPattern& pt = t.c.patterns[p];
    const int R = static_cast<int>(pt.rows.size()), rc = static_cast<int>(t.nchk[p]);
    CHECK(g.nrows[p] == static_cast<uint32_t>(R) && g.cmask[p] == (rc ? (1u << rc) - 1u : 0u));
    std::vector<std::vector<uint8_t>> G;
    for (int r = 0; r < R; ++r) G.push_back(g_row(k, m, pt.expect, pt.rows[static_cast<size_t>(r)]));
    // the arena: an expected source's column is G's, a compared source's the unit column of its row
    const uint8_t* base = g.arena.data() + p * g.tab_stride;
    for (size_t off = 0; off < g.tab_stride; ++off) {
      const size_t c = off / per, e = (off % per) / static_cast<size_t>(W), r = off % static_cast<size_t>(W);
      uint8_t want = 0;
      if (c < pt.delivered.size() && static_cast<int>(r) < R) {
        const int d = pt.delivered[c];
        const auto at = std::find(pt.expect.begin(), pt.expect.end(), d);
        const uint8_t coef = at != pt.expect.end() ? G[r][static_cast<size_t>(at - pt.expect.begin())]
                                                   : static_cast<uint8_t>(d == pt.rows[r] ? 1 : 0);
        CHECK(at == pt.expect.end() || coef != 0);
        want = slow_mul(coef, static_cast<uint8_t>(e < 16 ? e : (e - 16) << 4));
      }
      CHECK(base[off] == want);
    }
    // the locate block
    const uint8_t* blk = t.loc.data() + p * t.stride;
    for (int j = 0; j < k; ++j) CHECK(blk[kLocMap + static_cast<size_t>(j)] == pt.expect[static_cast<size_t>(j)]);
    for (int x = 0; x < rc; ++x) CHECK(blk[kLocMap + static_cast<size_t>(k + x)] == pt.rows[static_cast<size_t>(x)]);
    for (int j = 0; j < k; ++j)
      for (int r = 0; r < kLocateRows; ++r)
        CHECK(blk[kLocG + static_cast<size_t>(j) * kLocateRows + static_cast<size_t>(r)] ==
              (r < R ? G[static_cast<size_t>(r)][static_cast<size_t>(j)] : 0));
    int named = 0;
    for (int q = 0; q < 256; ++q) {
      const uint8_t j = blk[kLocRatio + static_cast<size_t>(q)];
      if (j == 0xff) continue;
      ++named;
      CHECK(rc >= 2 && j < k);
      CHECK(slow_mul(static_cast<uint8_t>(q), G[0][j]) == G[1][j]);  // q = G[1][j] / G[0][j]
    }
    CHECK(named == (rc >= 2 ? k : 0));  // pairwise distinct ratios: E is MDS
  }
}

void mul_word() {
  for (unsigned g = 0; g < 256; ++g)
    for (unsigned b = 0; b < 256; ++b) {
      const uint32_t w = b | ((b ^ 0x5au) << 8) | (((b * 7u) & 0xffu) << 16) | ((255u - b) << 24);
      const uint32_t o = repair_mul_word(g, w);
      for (int j = 0; j < 4; ++j)
        CHECK(((o >> (8 * j)) & 0xffu) == slow_mul(static_cast<uint8_t>(g), static_cast<uint8_t>(w >> (8 * j))));
    }
}

void layout() {
  const int k = 10, m = 4;
  const std::vector<int> first = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, last = {4, 5, 6, 7, 8, 9, 10, 11, 12, 13};
  const std::vector<int> mix = {0, 2, 3, 5, 6, 8, 9, 10, 12, 13};
  const std::vector<Stripe> st = {
      {first, {10}, {11, 12, 13}, {0, 11}, {0, 11}, 17},        // wanted 10 sorts before the compared shards
      {last, {1}, {0, 2, 3}, {13, 4, 3}, {}, 8192},             // compared on both sides of the wanted shard
      {first, {}, {10, 11, 12, 13}, {}, {}, 99},                // 4 + 0 rows, nothing delivered: scanned
      {mix, {1, 11}, {4, 7}, {0, 2, 7}, {7}, 8193},             // two check rows: nothing is repaired
      {first, {10}, {13, 12, 11}, {11, 0}, {}, 5},              // stripe 0's pattern again
      {mix, {}, {}, {0, 2, 12}, {}, 0},                         // no row: in no launch, size 0 is fine
      {first, {10, 11}, {}, {}, {}, 0},                         // wanted alone, nothing delivered: in no launch
      {first, {11}, {}, {3}, {3}, 40000},                       // no check row: an ordinary decode
  };
  DecodeRepairTables t;
  CHECK(build(k, m, st, t) == DecodeRepairError::kOk);
  CHECK(t.c.pat[0] == 0 && t.c.pat[1] == 1 && t.c.pat[2] == 2 && t.c.pat[3] == 3 && t.c.pat[4] == 0 && t.c.pat[7] == 4);
  CHECK(!t.c.has[5] && !t.c.has[6] && t.c.P() == 5);
  CHECK(t.c.patterns[0].rows == (std::vector<int>{11, 12, 13, 10}));
  CHECK(t.c.patterns[1].rows == (std::vector<int>{0, 2, 3, 1}));
  CHECK(t.c.patterns[3].rows == (std::vector<int>{4, 7, 1, 11}));
  CHECK(t.c.groups[0].cmask == (std::vector<uint32_t>{7, 7, 15, 3, 0}));
  CHECK(t.nchk == (std::vector<uint32_t>{3, 3, 4, 2, 0}));
  CHECK(fix_slots(k) == 26 && fix_slots(1) == 17);
  check_tables(k, m, st, t);
  // nothing in a launch: no group, no pattern
  const std::vector<Stripe> idle = {st[5], st[6]};
  CHECK(build(k, m, idle, t) == DecodeRepairError::kOk);
  CHECK(t.c.groups.empty() && t.c.P() == 0 && t.loc.empty() && t.c.map.ntiles == 0);
  check_tables(k, m, idle, t);
}

void refusals() {
  const int k = 4, m = 2;
  auto go = [&](int kk, int mm, const std::vector<Stripe>& st) {
    DecodeRepairTables t;
    return build(kk, mm, st, t);
  };
  const Stripe good = {{0, 1, 2, 3}, {4}, {5}, {0, 5}, {0, 5}, 16};
  CHECK(go(k, m, {good}) == DecodeRepairError::kOk);
  const Stripe few = {{0, 1, 2}, {4}, {}, {0}, {}, 16}, many = {{0, 1, 2, 3, 4}, {5}, {}, {0}, {}, 16};
  const Stripe in_unexpected = {{0, 1, 2, 3}, {5}, {}, {4}, {}, 16}, in_wanted = {{0, 1, 2, 3}, {4}, {5}, {4}, {}, 16};
  const Stripe dst_expected = {{0, 1, 2, 3}, {3}, {}, {0}, {}, 16}, chk_expected = {{0, 1, 2, 3}, {}, {3}, {0}, {}, 16};
  const Stripe chk_and_dst = {{0, 1, 2, 3}, {4}, {4}, {0}, {}, 16};
  const Stripe fix_wanted = {{0, 1, 2, 3}, {4}, {5}, {0}, {4}, 16}, fix_unused = {{0, 1, 2, 3}, {}, {5}, {0}, {4}, 16};
  const Stripe zero = {{0, 1, 2, 3}, {}, {4}, {0}, {}, 0};
  const Stripe zero_scan = {{0, 1, 2, 3}, {}, {4}, {}, {}, 0};  // a repair plan is final
  const Stripe zero_idle = {{0, 1, 2, 3}, {4}, {}, {}, {}, 0};
  CHECK(go(k, m, {few}) == DecodeRepairError::kTooFewShards);
  CHECK(go(k, m, {many}) == DecodeRepairError::kArg);
  for (const Stripe& s : {in_unexpected, in_wanted, dst_expected, chk_expected, chk_and_dst, fix_wanted, fix_unused}) {
    CHECK(go(k, m, {s}) == DecodeRepairError::kArg);
    CHECK(go(k, m, {zero, s}) == DecodeRepairError::kArg);                // before the sizes
    CHECK(go(k, m, {zero, s, few}) == DecodeRepairError::kTooFewShards);  // after the expected counts
  }
  CHECK(go(k, m, {zero}) == DecodeRepairError::kNoData);
  CHECK(go(k, m, {zero_scan}) == DecodeRepairError::kNoData);
  CHECK(go(k, m, {zero_idle, good}) == DecodeRepairError::kOk);
  CHECK(go(k, m, {many, few}) == DecodeRepairError::kArg);  // within a check, the first stripe
  CHECK(go(k, m, {few, many}) == DecodeRepairError::kTooFewShards);
  // the row limit: 16 rows pass, 17 are refused -- after a misplaced pointer, before a zero size
  std::vector<int> e10, w8, c8, c9;
  for (int i = 0; i < 10; ++i) e10.push_back(i);
  for (int i = 10; i < 18; ++i) w8.push_back(i);
  for (int i = 18; i < 26; ++i) c8.push_back(i);
  c9 = c8;
  c9.push_back(26);
  const Stripe rows16 = {e10, w8, c8, {0}, {}, 16}, rows17 = {e10, w8, c9, {0}, {}, 16};
  Stripe rows17_zero = rows17, rows17_fix = rows17, ok_zero = rows16;
  rows17_zero.size = 0;
  rows17_fix.fix = {10};
  ok_zero.size = 0;
  CHECK(go(10, 20, {rows16}) == DecodeRepairError::kOk);
  CHECK(go(10, 20, {rows17}) == DecodeRepairError::kUnsupported);
  CHECK(go(10, 20, {rows17_zero}) == DecodeRepairError::kUnsupported);
  CHECK(go(10, 20, {ok_zero, rows17}) == DecodeRepairError::kUnsupported);
  CHECK(go(10, 20, {rows17_fix}) == DecodeRepairError::kArg);
  CHECK(go(10, 20, {rows16, rows17_fix}) == DecodeRepairError::kArg);
  // 17 rows with no stripe in a launch are refused all the same
  Stripe idle17 = rows17;
  idle17.compared.clear();
  idle17.wanted = c9;
  idle17.wanted.insert(idle17.wanted.end(), w8.begin(), w8.end());
  idle17.delivered.clear();
  CHECK(go(10, 20, {idle17}) == DecodeRepairError::kUnsupported);
}

// One byte column of one stripe as the kernel forms it: the final launch delivers `now`, the
// rows' old bytes (merge mode) are what earlier launches left; returns the verdict and fills the
// wanted bytes, the position and the value. NW words of four rows each, as the RT instances.
template <int NW>
uint32_t model_column(const DecodeRepairTables& t, uint32_t p, const std::vector<uint8_t>& shard,
                      const std::vector<int>& now, const std::vector<uint8_t>& old, bool store,
                      std::vector<uint8_t>& wanted, uint32_t& pos, uint32_t& val) {
  const DecodeCheckPattern& pt = t.c.patterns[p];
  const int R = static_cast<int>(pt.rows.size()), rc = static_cast<int>(t.nchk[p]);
  CHECK(R <= NW * 4);
  (void)now;
  uint32_t s[NW] = {0};
  for (int r = 0; r < R; ++r) {
    uint8_t v = 0;
    for (size_t c = 0; c < pt.delivered.size(); ++c)
      v ^= slow_mul(pt.C.at(r, static_cast<int>(c)), shard[static_cast<size_t>(pt.delivered[c])]);
    if (!store) v ^= old[static_cast<size_t>(r)];
    s[r >> 2] |= static_cast<uint32_t>(v) << (8 * (r & 3));
  }
  pos = val = 0;
  const uint32_t v = repair_column(s, rc, R, t.c.k, t.gf.data(), t.loc.data() + p * t.stride, pos, val);
  wanted.clear();
  for (int r = rc; r < R; ++r) wanted.push_back(static_cast<uint8_t>(locate_byte(s, r)));
  return v;
}

// RS(k, m) with rc compared and w wanted shards. Expected: a seeded k-set with parity shards in
// it. Store mode delivers everything in the one launch; merge mode delivers a seeded half of the
// shards with the plan and finds the other half's terms in the rows (computed here from
// decode_plan's rows, not from the tables).
template <int NW>
void rule(int k, int m, int rc, int w, bool store, uint32_t seed) {
  std::mt19937 rng(seed);
  const int n = k + m;
  std::vector<int> all(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) all[static_cast<size_t>(i)] = i;
  std::shuffle(all.begin(), all.end(), rng);
  Stripe s;
  s.expect.assign(all.begin(), all.begin() + k);
  s.compared.assign(all.begin() + k, all.begin() + k + rc);
  s.wanted.assign(all.begin() + k + rc, all.begin() + k + rc + w);
  s.size = 16;
  std::vector<int> feed = s.expect;
  feed.insert(feed.end(), s.compared.begin(), s.compared.end());
  std::vector<int> earlier;
  if (!store) {
    std::shuffle(feed.begin(), feed.end(), rng);
    earlier.assign(feed.begin() + static_cast<ptrdiff_t>(feed.size() / 2), feed.end());
    feed.resize(feed.size() / 2);
  }
  s.delivered = feed;
  DecodeRepairTables t;
  CHECK(build(k, m, {s}, t) == DecodeRepairError::kOk);
  check_tables(k, m, {s}, t);
  const DecodeCheckPattern& pt = t.c.patterns[0];
  const int R = rc + w;
  std::vector<std::vector<uint8_t>> G;
  for (int r = 0; r < R; ++r) G.push_back(g_row(k, m, pt.expect, pt.rows[static_cast<size_t>(r)]));
  Mat E;
  CHECK(encode_matrix(k, m, E));
  // the rows' bytes before the final launch, for the shards as delivered
  auto old_rows = [&](const std::vector<uint8_t>& shard) {
    std::vector<uint8_t> old(static_cast<size_t>(R), 0);
    for (int r = 0; r < R; ++r)
      for (int i : earlier) {
        const auto at = std::find(pt.expect.begin(), pt.expect.end(), i);
        if (at != pt.expect.end()) old[static_cast<size_t>(r)] ^= slow_mul(G[static_cast<size_t>(r)][static_cast<size_t>(at - pt.expect.begin())], shard[static_cast<size_t>(i)]);
        else if (r < rc && pt.rows[static_cast<size_t>(r)] == i) old[static_cast<size_t>(r)] ^= shard[static_cast<size_t>(i)];
      }
    return old;
  };
  // what a reconstruct from the expected shards as delivered gives for the wanted rows
  auto as_computed = [&](const std::vector<uint8_t>& shard) {
    std::vector<uint8_t> out;
    for (int r = rc; r < R; ++r) {
      uint8_t v = 0;
      for (int j = 0; j < k; ++j) v ^= slow_mul(G[static_cast<size_t>(r)][static_cast<size_t>(j)], shard[static_cast<size_t>(pt.expect[static_cast<size_t>(j)])]);
      out.push_back(v);
    }
    return out;
  };
  for (int round = 0; round < 3; ++round) {
    // a true codeword's column
    std::vector<uint8_t> data(static_cast<size_t>(k)), truth(static_cast<size_t>(n), 0);
    for (auto& d : data) d = static_cast<uint8_t>(rng());
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < k; ++j) truth[static_cast<size_t>(i)] ^= slow_mul(E.at(i, j), data[static_cast<size_t>(j)]);
    std::vector<uint8_t> true_wanted;
    for (int r = rc; r < R; ++r) true_wanted.push_back(truth[static_cast<size_t>(pt.rows[static_cast<size_t>(r)])]);
    std::vector<uint8_t> got;
    uint32_t pos = 0, val = 0;
    // clean
    CHECK(model_column<NW>(t, 0, truth, feed, old_rows(truth), store, got, pos, val) == kLocateClean);
    CHECK(got == true_wanted && as_computed(truth) == true_wanted);
    // every single error: positions 0..k-1 are expected shards, k..k+rc-1 compared ones
    for (int at = 0; at < k + rc; ++at) {
      const int shard = at < k ? pt.expect[static_cast<size_t>(at)] : pt.rows[static_cast<size_t>(at - k)];
      for (unsigned e = 1; e < 256; ++e) {
        std::vector<uint8_t> bad = truth;
        bad[static_cast<size_t>(shard)] ^= static_cast<uint8_t>(e);
        const uint32_t v = model_column<NW>(t, 0, bad, feed, old_rows(bad), store, got, pos, val);
        if (rc >= 3) {
          CHECK(v == static_cast<uint32_t>(shard) && pos == static_cast<uint32_t>(at) && val == e);
          CHECK(got == true_wanted);
          CHECK(static_cast<uint8_t>(bad[static_cast<size_t>(shard)] ^ val) == truth[static_cast<size_t>(shard)]);
        } else {
          CHECK(v == kLocateUnexplained && got == as_computed(bad));  // the gate: nothing is repaired
        }
      }
    }
    // 2..rc-1 errors: unexplained (the code over the examined shards has distance rc + 1), and the
    // wanted bytes as computed
    for (int ne = 2; ne < rc; ++ne)
      for (int trial = 0; trial < 200; ++trial) {
        std::vector<int> at(static_cast<size_t>(k + rc));
        for (int i = 0; i < k + rc; ++i) at[static_cast<size_t>(i)] = i;
        std::shuffle(at.begin(), at.end(), rng);
        std::vector<uint8_t> bad = truth;
        for (int q = 0; q < ne; ++q) {
          const int a = at[static_cast<size_t>(q)];
          const int shard = a < k ? pt.expect[static_cast<size_t>(a)] : pt.rows[static_cast<size_t>(a - k)];
          bad[static_cast<size_t>(shard)] ^= static_cast<uint8_t>(1 + rng() % 255);
        }
        CHECK(model_column<NW>(t, 0, bad, feed, old_rows(bad), store, got, pos, val) == kLocateUnexplained);
        CHECK(got == as_computed(bad));
      }
  }
}

}  // namespace

int main() {
  mul_word();
  layout();
  refusals();
  uint32_t seed = 4242;
  for (const bool store : {false, true}) {
    rule<1>(10, 4, 3, 1, store, seed++);
    rule<1>(10, 4, 4, 0, store, seed++);
    rule<4>(10, 4, 3, 1, store, seed++);  // a wider instance serves fewer rows
    rule<1>(4, 2, 2, 0, store, seed++);   // r' = 2: flagged, nothing repaired
    rule<1>(4, 2, 1, 1, store, seed++);   // r' = 1
    rule<1>(6, 3, 3, 0, store, seed++);
    rule<1>(6, 3, 2, 1, store, seed++);
    rule<2>(10, 8, 4, 4, store, seed++);
    rule<4>(20, 12, 3, 9, store, seed++);
    rule<4>(10, 20, 8, 8, store, seed++);
    rule<1>(1, 3, 3, 0, store, seed++);
    rule<1>(3, 2, 2, 0, store, seed++);
  }
  std::printf("decode_repair_host_test ok\n");
  return 0;
}
