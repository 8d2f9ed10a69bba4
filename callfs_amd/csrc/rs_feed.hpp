// Feed launches: one delivered shard of one stripe into the stripe's resident
// rows. Single-source, so every coefficient is wave-uniform and the kernel is the v_perm form of
// rs_apply_vec (§5.2, §5.3): `selectors` once per input dword, gf_mul4 per row, the shard's block
// of [R][5] table words read through the constant address space into SGPRs. No LDS, no table
// prologue, no tile map, no pattern tables: a launch names its source, its table block and its
// rows by argument. One 16-byte vector per lane, kFeedBlock lanes per block: block b owns bytes
// [b * kFeedTileBytes, (b + 1) * kFeedTileBytes) of the source and of every row. The source
// vector is loaded first; the rows then go four at a time (four loads in flight, then their four
// stores), which keeps the 16-row instances far below 128 VGPRs. Merge: row ^= c * src, and a row
// whose coefficient is 0 (every row but its own under a compared shard) is neither read nor
// written. STORE: row = c * src, no row byte is read, a zero coefficient stores zeros. Row
// accesses and the source load are non-temporal, plain unaligned 16-byte accesses at any
// address. The S % 16 tail is done by bytes in the last block, one byte per lane, as merge_tail
// does; S < 16 is one block that is all tail. Included by rs_mixed.hip alone.
#pragma once

#include "rs_apply.hpp"

namespace callfs {
namespace dev {

constexpr int kFeedBlock = 256;
static_assert(kFeedBlock * 16 == static_cast<int>(kFeedTileBytes), "one 16-byte vector per lane");

// non-temporal loads and stores, nothing else of a Policy is read
using FeedPolicy = Policy<1, 1, true, true, false, kFeedBlock>;

// Row r's pointer: a kernel argument up to 8 rows, the feed object's device table above.
template <int RT>
__device__ __forceinline__ uint8_t* feed_row(const ApplyArgs& a, const FeedRows<RT>& x, int r) {
  if constexpr (RT > 8) return as_const(a.out_tab)[r];
  else return x.row[r];
}

// An RT instance serves every feed object of up to RT rows; rows >= a.R are never touched.
// a.S, a.nvec = S / 16, a.R, a.tabs (the delivered shard's block) and, for RT 16, a.out_tab are
// what the kernel reads of `a`.
template <int RT, bool STORE>
__global__ __launch_bounds__(kFeedBlock) void rs_feed(ApplyArgs a, FeedRows<RT> x) {
  using P = FeedPolicy;
  const cptr<uint32_t> tabs = as_const(a.tabs);
  const int R = a.R;
  const uint64_t v0 = static_cast<uint64_t>(blockIdx.x) * kFeedBlock + threadIdx.x;
  if (v0 < a.nvec) {
    // the source goes out ahead of the first row load; v0 < nvec: bytes [16 v0, 16 v0 + 16) lie
    // below S in the source and in every row
    const uint4 s = load16<P>(reinterpret_cast<const uint4*>(x.src) + v0);
    const Sel sel[4] = {selectors(s.x), selectors(s.y), selectors(s.z), selectors(s.w)};
#pragma unroll
    for (int r0 = 0; r0 < RT; r0 += 4) {
      if (r0 >= R) break;  // wave-uniform
      uint4 y[4];
      if constexpr (!STORE) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          y[q] = make_uint4(0, 0, 0, 0);
          // c == 0 exactly when the word that holds c * 1 is 0
          if (r0 + q < R && tabs[(r0 + q) * 5] != 0)
            y[q] = load16<P>(reinterpret_cast<const uint4*>(feed_row<RT>(a, x, r0 + q)) + v0);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + q;
        if (r >= R) continue;                        // wave-uniform
        if (!STORE && tabs[r * 5] == 0) continue;  // wave-uniform: nothing to add
        uint32_t o[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) o[w] = fma1(STORE ? 0u : word(y[q], w), gf_mul4(sel[w], tabs + r * 5));
        store16<P>(reinterpret_cast<uint4*>(feed_row<RT>(a, x, r)) + v0, make_uint4(o[0], o[1], o[2], o[3]));
      }
    }
  }
  // the S % 16 tail: its bytes lie in the last block's range, and that block's last 16 lanes take
  // one each (after their vector, if they had one); byte b < S in the source and in every row
  if (blockIdx.x + 1 == gridDim.x && threadIdx.x >= kFeedBlock - 16) {
    const uint64_t b = a.nvec * 16 + (threadIdx.x - (kFeedBlock - 16));
    if (b < a.S) {
      const Sel sb = selectors(x.src[b]);
      for (int r = 0; r < R && r < RT; ++r) {
        if (!STORE && tabs[r * 5] == 0) continue;
        uint8_t* row = feed_row<RT>(a, x, r);
        const uint32_t v = fma1(STORE ? 0u : row[b], gf_mul4(sb, tabs + r * 5));
        row[b] = static_cast<uint8_t>(v);
      }
    }
  }
}

}  // namespace dev
}  // namespace callfs
