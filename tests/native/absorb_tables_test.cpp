// Host-side tables of absorb objects and the book of encode sessions on the CPU,
// built with g++ -fsanitize=address,undefined by tests/test_native_absorb.py:
//  - every arena word equals perm_tables of the encoding matrix's entry E[k + j][i], and every
//    block, evaluated over all 256 inputs, is a bit-by-bit GF(2^8) multiply by that entry;
//  - the refusals in the stated order, RS(10,20) and a 17-row profile among them;
//  - absorb_plan: at most three intervals, pairwise disjoint columns, every byte of the range in
//    exactly one of them and no other byte, the running block counts;
//  - a scalar model of the launches: every launch's intervals applied byte by byte to zeroed rows,
//    over shuffled sets of ranges that cover [0, L) exactly once, ends in a straightforward encode
//    of the padded body, for the shapes of the GPU tests;
//  - the book: overlap, gap, out-of-range and after-finish refusals, coverage complete only at
//    exactly [0, L), shuffled ranges merging to one interval, L < k, the route of a piece and the
//    cutting of a feed into slot-sized pieces.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "absorb_tables.hpp"
#include "gf256.hpp"
#include "host_encode_session.hpp"

using namespace callfs;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

constexpr uint64_t T = 4096;

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

// what gf_mul4 computes for one byte from a block of five words
uint8_t perm_mul(const uint32_t* w, unsigned x) {
  auto byte = [](uint32_t lo, uint32_t hi, unsigned e) {
    return static_cast<uint8_t>((e < 4 ? lo >> (8 * e) : hi >> (8 * (e - 4))) & 0xffu);
  };
  return static_cast<uint8_t>(byte(w[0], w[1], x & 7u) ^ byte(w[2], w[3], (x >> 3) & 7u) ^
                              byte(w[4], w[4], x >> 6));
}

void check_tables(int k, int m) {
  AbsorbTables t;
  CHECK(build_absorb_tables(k, m, 17, t) == AbsorbError::kOk);
  CHECK(t.k == k && t.m == m && t.P.rows == m && t.P.cols == k);
  CHECK(t.block_words() == static_cast<size_t>(m) * kTabWords);
  CHECK(t.arena.size() == static_cast<size_t>(k) * t.block_words());
  Mat E;
  CHECK(encode_matrix(k, m, E));
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < m; ++j) {
      const uint8_t c = E.at(k + j, i);
      CHECK(t.P.at(j, i) == c);
      uint32_t want[kTabWords];
      perm_tables(c, want);
      const uint32_t* w = &t.arena[static_cast<size_t>(i) * t.block_words() + static_cast<size_t>(j) * kTabWords];
      for (int q = 0; q < kTabWords; ++q) CHECK(w[q] == want[q]);
      for (unsigned x = 0; x < 256; ++x) CHECK(perm_mul(w, x) == slow_mul(c, static_cast<uint8_t>(x)));
    }
}

void check_refusals() {
  AbsorbTables t;
  // more than 16 rows, before a zero size
  CHECK(build_absorb_tables(10, 20, 0, t) == AbsorbError::kUnsupported);
  CHECK(build_absorb_tables(10, 20, 16, t) == AbsorbError::kUnsupported);
  CHECK(build_absorb_tables(10, 17, 0, t) == AbsorbError::kUnsupported);  // 17 rows
  CHECK(build_absorb_tables(239, 17, 16, t) == AbsorbError::kUnsupported);
  CHECK(build_absorb_tables(10, 16, 0, t) == AbsorbError::kNoData);
  CHECK(build_absorb_tables(10, 4, 0, t) == AbsorbError::kNoData);
  CHECK(build_absorb_tables(10, 16, 1, t) == AbsorbError::kOk);
  // a launch's range: empty, or outside [0, k * S)
  AbsorbPlan p;
  CHECK(!absorb_plan(10, 16, 0, 0, p));
  CHECK(!absorb_plan(10, 16, 160, 1, p));
  CHECK(!absorb_plan(10, 16, 159, 2, p));
  CHECK(!absorb_plan(10, 16, 0, 161, p));
  CHECK(!absorb_plan(10, 16, ~uint64_t{0}, 2, p));
  CHECK(!absorb_plan(10, 0, 0, 1, p));
  CHECK(absorb_plan(10, 16, 159, 1, p) && p.n == 1 && p.grid() == 1);
  CHECK(absorb_plan(10, 16, 0, 160, p) && p.n == 1 && p.iv[0].shard0 == 0 && p.iv[0].shard1 == 9);
}

// One launch of the scalar model: the plan's intervals byte by byte. `hits` counts how often a
// body byte was read.
void model_launch(const AbsorbTables& t, size_t S, uint64_t off, uint64_t len, const std::vector<uint8_t>& body,
                  std::vector<std::vector<uint8_t>>& rows, std::vector<int>& hits, int want_intervals = 0) {
  AbsorbPlan p;
  CHECK(absorb_plan(t.k, S, off, len, p));
  CHECK(p.n >= 1 && p.n <= kAbsorbMaxIntervals);
  if (want_intervals) CHECK(p.n == want_intervals);
  uint64_t blocks = 0, bytes = 0;
  for (int q = 0; q < kAbsorbMaxIntervals; ++q) {
    if (q < p.n) {
      const AbsorbInterval& v = p.iv[q];
      CHECK(v.col0 < v.col1 && v.col1 <= S && v.shard0 >= 0 && v.shard0 <= v.shard1 && v.shard1 < t.k);
      if (q) CHECK(p.iv[q - 1].col1 <= v.col0);  // ascending, disjoint columns
      blocks += (v.col1 - v.col0 + T - 1) / T;
      for (uint64_t c = v.col0; c < v.col1; ++c)
        for (int i = v.shard0; i <= v.shard1; ++i) {
          const uint64_t x = static_cast<uint64_t>(i) * S + c;
          CHECK(x >= off && x < off + len);  // no byte is read outside [src, src + len)
          ++hits[static_cast<size_t>(x)];
          ++bytes;
          for (int j = 0; j < t.m; ++j)
            rows[static_cast<size_t>(j)][static_cast<size_t>(c)] ^= gf().mul[t.P.at(j, i)][body[static_cast<size_t>(x)]];
        }
    }
    CHECK(p.end[q] == blocks);
  }
  CHECK(bytes == len);  // every byte of the range, once
  CHECK(p.grid() == blocks);
}

// ranges that cover [0, L) exactly once: `special` (clipped to L, may be empty) and pieces of
// `piece` bytes over the rest
std::vector<std::pair<uint64_t, uint64_t>> cover(uint64_t L, uint64_t piece, std::pair<uint64_t, uint64_t> special) {
  std::vector<std::pair<uint64_t, uint64_t>> r;
  uint64_t s0 = std::min(special.first, L), s1 = std::min(special.first + special.second, L);
  for (uint64_t at = 0; at < s0; at += piece) r.push_back({at, std::min(piece, s0 - at)});
  if (s1 > s0) r.push_back({s0, s1 - s0});
  for (uint64_t at = s1; at < L; at += piece) r.push_back({at, std::min(piece, L - at)});
  return r;
}

void check_model(int k, int m, size_t S, uint64_t L, std::mt19937& rng) {
  CHECK((L + static_cast<uint64_t>(k) - 1) / static_cast<uint64_t>(k) == S);
  AbsorbTables t;
  CHECK(build_absorb_tables(k, m, S, t) == AbsorbError::kOk);
  std::vector<uint8_t> body(static_cast<size_t>(k) * S, 0);
  for (uint64_t x = 0; x < L; ++x) body[static_cast<size_t>(x)] = static_cast<uint8_t>(rng());
  // the straightforward encode of the padded body
  Mat E;
  CHECK(encode_matrix(k, m, E));
  std::vector<std::vector<uint8_t>> want(static_cast<size_t>(m), std::vector<uint8_t>(S, 0));
  for (int j = 0; j < m; ++j)
    for (size_t c = 0; c < S; ++c)
      for (int i = 0; i < k; ++i)
        want[static_cast<size_t>(j)][c] ^= slow_mul(E.at(k + j, i), body[static_cast<size_t>(i) * S + c]);
  std::vector<std::vector<std::pair<uint64_t, uint64_t>>> sets;
  sets.push_back({{0, L}});
  sets.push_back(cover(L, S, {0, 0}));
  if (S <= 17) sets.push_back(cover(L, 1, {0, 0}));
  for (uint64_t piece : {uint64_t{7}, uint64_t{16}, uint64_t{100}, static_cast<uint64_t>(S) + 3})
    sets.push_back(cover(L, piece, {0, 0}));
  sets.push_back(cover(L, S + 3, {0, 0}));
  std::shuffle(sets.back().begin(), sets.back().end(), rng);
  // three intervals: 2S + 5 bytes from column S - 2 of a shard
  const int three = static_cast<int>(sets.size());
  const bool has_three = k >= 4 && S >= 3 && (S - 2) + 2 * S + 5 <= L;
  if (has_three) sets.push_back(cover(L, S + 3, {S - 2, 2 * S + 5}));
  // two shards, the empty middle interval: S - 1 bytes from column S - 3
  const int two = static_cast<int>(sets.size());
  const bool has_two = k >= 2 && S >= 5 && (S - 3) + (S - 1) <= L;
  if (has_two) sets.push_back(cover(L, S + 3, {S - 3, S - 1}));
  for (size_t si = 0; si < sets.size(); ++si) {
    auto ranges = sets[si];
    if (static_cast<int>(si) >= three) std::shuffle(ranges.begin(), ranges.end(), rng);
    std::vector<std::vector<uint8_t>> rows(static_cast<size_t>(m), std::vector<uint8_t>(S, 0));
    std::vector<int> hits(static_cast<size_t>(k) * S, 0);
    for (const auto& r : ranges) {
      int n = 0;
      // (up to S = 5 the first shard's columns meet the last shard's: two intervals)
      if (has_three && S >= 6 && static_cast<int>(si) == three && r.first == S - 2 && r.second == 2 * S + 5) n = 3;
      if (has_two && static_cast<int>(si) == two && r.first == S - 3 && r.second == S - 1) n = 2;
      model_launch(t, S, r.first, r.second, body, rows, hits, n);
    }
    for (uint64_t x = 0; x < static_cast<uint64_t>(k) * S; ++x) CHECK(hits[static_cast<size_t>(x)] == (x < L ? 1 : 0));
    CHECK(rows == want);
  }
}

void check_book() {
  EncodeBook b;
  b.open(10, 397);
  CHECK(b.S == 40 && b.L == 397 && !b.complete());
  // empty, out of range
  CHECK(b.may_feed(0, 0) == RS_E_ARG);
  CHECK(b.may_feed(397, 1) == RS_E_ARG);
  CHECK(b.may_feed(396, 2) == RS_E_ARG);
  CHECK(b.may_feed(0, 398) == RS_E_ARG);
  CHECK(b.may_feed(~uint64_t{0}, 2) == RS_E_ARG);
  CHECK(b.may_feed(5, ~uint64_t{0}) == RS_E_ARG);
  CHECK(b.may_feed(100, 50) == RS_OK);
  b.note_feed(100, 50);
  // overlap at either end, inside, around
  CHECK(b.may_feed(99, 2) == RS_E_ARG && b.may_feed(149, 1) == RS_E_ARG && b.may_feed(120, 5) == RS_E_ARG);
  CHECK(b.may_feed(90, 100) == RS_E_ARG && b.may_feed(100, 50) == RS_E_ARG);
  // neighbours are fine
  CHECK(b.may_feed(99, 1) == RS_OK && b.may_feed(150, 1) == RS_OK);
  b.note_feed(150, 247);
  CHECK(b.fed.size() == 1 && b.fed[0].first == 100 && b.fed[0].second == 397 && !b.complete());
  b.note_feed(0, 99);
  CHECK(b.fed.size() == 2 && !b.complete() && b.fed_bytes() == 396);  // a gap of one byte
  CHECK(b.may_feed(98, 2) == RS_E_ARG && b.may_feed(99, 2) == RS_E_ARG);
  CHECK(b.may_feed(99, 1) == RS_OK);
  b.note_feed(99, 1);
  CHECK(b.complete() && b.fed.size() == 1);
  CHECK(b.may_feed(0, 1) == RS_E_ARG);
  b.finished = true;
  b.open(10, 397);
  CHECK(!b.finished && b.fed.empty());
  b.finished = true;
  CHECK(b.may_feed(0, 10) == RS_E_ARG);  // after a finish
  // coverage of [1, L) or [0, L - 1) alone is not complete
  b.open(4, 100);
  b.note_feed(1, 99);
  CHECK(!b.complete());
  b.open(4, 100);
  b.note_feed(0, 99);
  CHECK(!b.complete());
  b.note_feed(99, 1);
  CHECK(b.complete());
  // shuffled ranges merge to one interval
  std::mt19937 rng(518);
  for (int round = 0; round < 20; ++round) {
    const uint64_t L = 1 + rng() % 5000;
    b.open(10, L);
    auto ranges = cover(L, 1 + rng() % 97, {0, 0});
    std::shuffle(ranges.begin(), ranges.end(), rng);
    for (size_t at = 0; at < ranges.size(); ++at) {
      CHECK(!b.complete());
      CHECK(b.may_feed(ranges[at].first, ranges[at].second) == RS_OK);
      b.note_feed(ranges[at].first, ranges[at].second);
      CHECK(b.may_feed(ranges[at].first, ranges[at].second) == RS_E_ARG);
      for (size_t q = 1; q < b.fed.size(); ++q) CHECK(b.fed[q - 1].second < b.fed[q].first);  // sorted, merged
    }
    CHECK(b.complete() && b.fed.size() == 1);
  }
  // L < k: S = 1, the shards past L are all padding
  b.open(4, 2);
  CHECK(b.S == 1);
  CHECK(b.may_feed(2, 1) == RS_E_ARG);
  b.note_feed(1, 1);
  CHECK(!b.complete());
  b.note_feed(0, 1);
  CHECK(b.complete());
  // slots and pieces
  CHECK(encode_session_slot(2, 4u << 20) == 2 && encode_session_slot(10u << 20, 4u << 20) == (4u << 20));
  unsetenv("CALLFS_RS_ENCODE_SESSION_CHUNK");
  CHECK(encode_session_chunk() == (4u << 20));
  setenv("CALLFS_RS_ENCODE_SESSION_CHUNK", "1000", 1);
  CHECK(encode_session_chunk() == 1000);
  setenv("CALLFS_RS_ENCODE_SESSION_CHUNK", "0", 1);
  CHECK(encode_session_chunk() == 1);
  unsetenv("CALLFS_RS_ENCODE_SESSION_CHUNK");
  std::vector<EncodePiece> p;
  encode_pieces(7, 2500, 1000, p);  // 2.5 slots: three launches
  CHECK(p.size() == 3 && p[0].off == 7 && p[0].n == 1000 && p[1].off == 1007 && p[1].n == 1000 &&
        p[2].off == 2007 && p[2].n == 500);
  encode_pieces(0, 1000, 1000, p);
  CHECK(p.size() == 1 && p[0].n == 1000);
  encode_pieces(3, 1001, 1000, p);
  CHECK(p.size() == 2 && p[1].off == 1003 && p[1].n == 1);
  // the route is decided per piece, by the piece's size
  CHECK(feed_route(1000, 1000, false) == FeedRoute::kInPlace);
  CHECK(feed_route(1000, 1000, true) == FeedRoute::kDirect);
  CHECK(feed_route(1001, 1000, false) == FeedRoute::kStaged);
  CHECK(feed_route(1001, 1000, true) == FeedRoute::kStaged);
  CHECK(feed_route(1, 0, true) == FeedRoute::kStaged);
}

}  // namespace

int main() {
  const int profiles[][2] = {{10, 4}, {4, 2}, {3, 2}, {1, 3}, {16, 4}, {10, 8}, {20, 12}, {200, 16}};
  for (const auto& p : profiles) check_tables(p[0], p[1]);
  check_refusals();
  std::mt19937 rng(20518);
  for (size_t S : {size_t{1}, size_t{5}, size_t{15}, size_t{16}, size_t{17}, size_t{40}, size_t{1023}, size_t{T - 1},
                   size_t{T}, size_t{T + 1}, size_t{T + 16}, size_t{2 * T + 83}}) {
    check_model(10, 4, S, 10 * S - 7, rng);
    check_model(10, 4, S, 10 * S, rng);
  }
  const int others[][2] = {{1, 3}, {3, 2}, {4, 2}, {16, 4}, {10, 8}, {20, 12}, {64, 16}};
  for (const auto& p : others)
    for (size_t S : {size_t{17}, size_t{T + 16}}) {
      const uint64_t pad = static_cast<uint64_t>(std::min(7, p[0] - 1));
      check_model(p[0], p[1], S, static_cast<uint64_t>(p[0]) * S - pad, rng);
    }
  check_model(4, 2, 1, 2, rng);  // "hi": L < k
  check_book();
  std::printf("absorb_tables_test ok\n");
  return 0;
}
