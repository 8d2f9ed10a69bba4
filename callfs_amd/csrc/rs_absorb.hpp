// Absorb launches: one byte range of an object's body into the object's
// resident parity rows. The range covers, at every column it touches, a run of consecutive data
// shards; absorb_plan (absorb_tables.hpp) cuts the columns into at most three intervals with one
// run each. The kernel is the v_perm form of rs_feed (§5.2, §5.17) with a loop over the run: per
// lane one 16-byte column vector, `selectors` once per input dword and gf_mul4 per row, the
// products XORed into R accumulators of four dwords that stay in registers, shard i's block of
// [R][5] table words read through the constant address space into SGPRs. The next shard's vector
// is in flight while the current one is multiplied. After the loop the rows go four at a time as
// in rs_feed (four loads in flight, XOR, four stores), so each row is read and written once
// however many shards the range covers. No LDS, no table prologue, no tile map: block b finds its
// interval by comparing blockIdx.x with the intervals' running block counts (wave-uniform) and
// owns kFeedTileBytes columns of it. Source loads and row accesses are non-temporal, plain
// unaligned 16-byte accesses. An interval's (col1 - col0) % 16 tail is done by bytes in the
// interval's last block, one byte per lane in its last 16 lanes; an interval shorter than 16
// columns is one block that is all tail. Included by rs_mixed.hip alone.
#pragma once

#include "rs_feed.hpp"

namespace callfs {
namespace dev {

static_assert(kAbsorbTileBytes == kFeedTileBytes, "an absorb block covers a feed block's columns");

template <int RT>
__device__ __forceinline__ uint8_t* absorb_row(const ApplyArgs& a, const AbsorbRows<RT>& x, int r) {
  if constexpr (RT > 8) return as_const(a.out_tab)[r];
  else return x.row[r];
}

// An RT instance serves every object of up to RT rows; rows >= a.R are never touched. a.S (the
// shard size), a.R, a.tabs (the arena) and, for RT 16, a.out_tab are what the kernel reads of `a`.
// Bounds: a vector access happens only for c + 16 <= col1 and a byte access only for c < col1, so
// every row access lies in [row + col0, row + col1); byte (i, c) of an interval is byte
// i * S + c of the body and lies in [off, off + len), so every source access lies in
// [src, src + len).
template <int RT>
__global__ __launch_bounds__(kFeedBlock) void rs_absorb(ApplyArgs a, AbsorbRows<RT> x) {
  using P = FeedPolicy;
  const int R = a.R;
  const uint32_t b = blockIdx.x;
  // the block's interval, all wave-uniform
  const bool q1 = b >= x.end[0], q2 = b >= x.end[1];
  const uint64_t col0 = q2 ? x.iv[2].col0 : q1 ? x.iv[1].col0 : x.iv[0].col0;
  const uint64_t col1 = q2 ? x.iv[2].col1 : q1 ? x.iv[1].col1 : x.iv[0].col1;
  const int shard0 = q2 ? x.iv[2].shard0 : q1 ? x.iv[1].shard0 : x.iv[0].shard0;
  const int shard1 = q2 ? x.iv[2].shard1 : q1 ? x.iv[1].shard1 : x.iv[0].shard1;
  const uint32_t first = q2 ? x.end[1] : q1 ? x.end[0] : 0u;
  const uint32_t last = q2 ? x.end[2] : q1 ? x.end[1] : x.end[0];
  const uint64_t nvec = (col1 - col0) / 16;
  const uint64_t v = static_cast<uint64_t>(b - first) * kFeedBlock + threadIdx.x;
  const size_t bw = static_cast<size_t>(R) * 5;  // words per shard block
  if (v < nvec) {
    const uint64_t c = col0 + v * 16;  // c + 16 <= col1
    // body byte (i, c) at src + (i * S + c - off)
    const uint8_t* s0 = x.src + (static_cast<uint64_t>(shard0) * a.S + c - x.off);
    auto ld = [&](int i) {
      return load16<P>(reinterpret_cast<const uint4*>(s0 + static_cast<uint64_t>(i - shard0) * a.S));
    };
    uint32_t acc[RT][4];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int w = 0; w < 4; ++w) acc[r][w] = 0;
    uint4 cur = ld(shard0);
#pragma unroll 1
    for (int i = shard0; i <= shard1; ++i) {
      uint4 nxt = cur;
      if (i < shard1) nxt = ld(i + 1);  // wave-uniform
      const cptr<uint32_t> t = as_const(a.tabs) + static_cast<size_t>(i) * bw;
      const Sel sel[4] = {selectors(cur.x), selectors(cur.y), selectors(cur.z), selectors(cur.w)};
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r < R) {  // wave-uniform
#pragma unroll
          for (int w = 0; w < 4; ++w) acc[r][w] = fma1(acc[r][w], gf_mul4(sel[w], t + r * 5));
        }
      }
      cur = nxt;
    }
#pragma unroll
    for (int r0 = 0; r0 < RT; r0 += 4) {
      if (r0 >= R) break;  // wave-uniform
      uint4 y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        y[q] = make_uint4(0, 0, 0, 0);
        if (r0 + q < R) y[q] = load16<P>(reinterpret_cast<const uint4*>(absorb_row<RT>(a, x, r0 + q) + c));
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + q;
        if (r >= R) continue;  // wave-uniform
        store16<P>(reinterpret_cast<uint4*>(absorb_row<RT>(a, x, r) + c),
                   make_uint4(y[q].x ^ acc[r][0], y[q].y ^ acc[r][1], y[q].z ^ acc[r][2], y[q].w ^ acc[r][3]));
      }
    }
  }
  // the interval's tail: its last block's last 16 lanes take one byte each (after their vector,
  // if they had one); c < col1
  if (b + 1 == last && threadIdx.x >= kFeedBlock - 16) {
    const uint64_t c = col0 + nvec * 16 + (threadIdx.x - (kFeedBlock - 16));
    if (c < col1) {
      uint32_t acc[RT];
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = 0;
      const uint8_t* s0 = x.src + (static_cast<uint64_t>(shard0) * a.S + c - x.off);
#pragma unroll 1
      for (int i = shard0; i <= shard1; ++i) {
        const Sel sb = selectors(s0[static_cast<uint64_t>(i - shard0) * a.S]);
        const cptr<uint32_t> t = as_const(a.tabs) + static_cast<size_t>(i) * bw;
#pragma unroll
        for (int r = 0; r < RT; ++r)
          if (r < R) acc[r] = fma1(acc[r], gf_mul4(sb, t + r * 5));
      }
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r >= R) continue;
        uint8_t* row = absorb_row<RT>(a, x, r);
        row[c] = static_cast<uint8_t>(row[c] ^ acc[r]);
      }
    }
  }
}

}  // namespace dev
}  // namespace callfs
