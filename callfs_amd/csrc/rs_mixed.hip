// Mixed launches: one launch group over a batch in which every stripe has
// its own erasure pattern. The kernels are the nibble-table LDS kernel of rs_apply.hpp with
// the tables and the compare mask chosen per block: tiles never straddle stripes, so a
// block reads its stripe's pattern p = pat[stripe] (a wave-uniform scalar load), stages
// pattern p's tables from the launch group's arena into LDS and takes vmask[p] as its
// verify mask. Input loop, lookups, accumulation, stores and compares are the helpers of
// rs_apply.hpp; existing kernel instances are untouched.
// Ragged launches run the same block body with the stripe, its tile and
// its shard size read per block from a tile map: one launch group over stripes of
// different shard sizes. Required launches (§5.10) are ragged launches that also read each
// pattern's row count; one host function, launch_ragged, enqueues both. Locate launches
// (§5.12) are required launches that compare every row and classify the mismatching byte
// columns into per-stripe, per-shard counts; the pair instances (§5.12.1) classify with
// locate_classify2 and add a column blamed on two shards into both shards' counts. Correct
// launches (§5.13) are locate launches that XOR the error value into the blamed shard's byte.
// Decode-repair launches (§5.16, rs_repair.hpp) are final decode-check launches that classify a
// mismatching column from their check rows and repair the wanted rows before storing them.
// Feed launches (§5.17, rs_feed.hpp) deliver one shard of one stripe into its resident rows: the
// v_perm form, selected by argument, with no tile map and no LDS.
// Absorb launches (§5.18, rs_absorb.hpp) fold one byte range of an object's body into its resident
// parity rows: the same form with a loop over the shards the range covers at a column.
#include <algorithm>
#include <array>

#include <hip/hip_ext.h>

#include "dispatch.hpp"
#include "launch_util.hpp"
#include "locate_tables.hpp"
#include "rs_apply.hpp"
#include "rs_check.hpp"
#include "rs_absorb.hpp"
#include "rs_feed.hpp"
#include "rs_merge.hpp"
#include "rs_update.hpp"

namespace callfs {

namespace dev {

// Ring of three input vectors for RT <= 8 (as LdsPolicy), with the Verify rows' compare
// loads issued 4 shards before the end of the loop for RT <= 4 (as LdsVerifyPolicy: almost
// every mixed launch compares rows); the unrolled 5-slot ring with SDWA table addresses for
// RT 9..16 (as LdsWidePolicy). Consecutive tile order.
using MixedPolicy4 = Policy<2, 1, true, true, false, 512, 2, 0, 0, false, 0, false, 0, 4>;
using MixedPolicy8 = Policy<2, 1, true, true, false, 512, 2, 0>;
using MixedPolicy16 = Policy<2, 1, true, true, false, 512, 4, 0, 1, false, false, true>;
template <int RT>
using MixedPolicy = typename std::conditional<
    (RT > 8), MixedPolicy16, typename std::conditional<(RT > 4), MixedPolicy8, MixedPolicy4>::type>::type;

// ---- locate ---------------------------------------------------------------
// XORs byte b into row r of an accumulator element (r static under an unrolled loop).
template <int RT>
__device__ __forceinline__ void lds_xor_byte(typename LdsAcc<RT>::T& t, int r, uint32_t b) {
  if constexpr (RT > 8) t.v[r >> 2] ^= b << (8 * (r & 3));
  else if constexpr (RT > 4) t ^= static_cast<uint64_t>(b) << (8 * r);
  else t ^= b << (8 * r);
}

// An accumulator element's syndromes, one per row, as the words the rule reads.
template <int RT>
__device__ __forceinline__ void locate_words(const typename LdsAcc<RT>::T& t, uint32_t (&s)[RT / 4]) {
  if constexpr (RT > 8) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = t.v[i];
  } else if constexpr (RT > 4) {
    s[0] = static_cast<uint32_t>(t);
    s[1] = static_cast<uint32_t>(t >> 32);
  } else {
    s[0] = t;
  }
}

// One byte column's verdict from its syndromes, one per row in the accumulator element.
// PAIR: by a pair plan's rule.
template <int RT, bool PAIR>
__device__ __forceinline__ uint32_t locate_column(const typename LdsAcc<RT>::T& t, int rows, int K,
                                                  const uint8_t* gf, const uint8_t* pt) {
  uint32_t s[RT / 4];
  locate_words<RT>(t, s);
  if constexpr (PAIR) return locate_classify2(s, rows, K, gf, pt);
  else return locate_classify(s, rows, K, gf, pt);
}

// A correct plan's column: locate_correct's verdict, and for a shard verdict
// the position in T = valid then cmp and the error value to XOR into that shard's byte.
template <int RT>
__device__ __forceinline__ uint32_t correct_column(const typename LdsAcc<RT>::T& t, int rows, int K,
                                                   const uint8_t* gf, const uint8_t* pt, uint32_t& pos,
                                                   uint32_t& value) {
  uint32_t s[RT / 4];
  locate_words<RT>(t, s);
  return locate_correct(s, rows, K, gf, pt, pos, value);
}

// The shard at position pos of a stripe's T: in_tab's slot pos, or out_tab's slot pos - K. The
// index differs from lane to lane, so these are plain global loads of the pointer tables (only
// lanes with something to repair come here). A correct plan's in_tab names writable shards.
__device__ __forceinline__ uint8_t* correct_shard(const ApplyArgs& a, uint32_t stripe, uint32_t out_stride,
                                                  uint32_t pos) {
  const uint32_t K = static_cast<uint32_t>(a.K);
  return pos < K ? const_cast<uint8_t*>(a.in_tab[static_cast<size_t>(stripe) * K + pos])
                 : a.out_tab[static_cast<size_t>(stripe) * out_stride + (pos - K)];
}

// Adds every lane's n (0..16) columns of verdict v (kLocateClean: none) into the stripe's
// bins: one 64-bit atomic per distinct verdict in the wave, issued by one lane. Sums are
// formed from ballots alone, so lanes that have left the kernel count as nothing; every lane
// still in the wave must arrive together (no barrier, no LDS). PAIR: a pair verdict's sum goes
// into both shards' bins, by the same lane.
template <bool PAIR>
__device__ __forceinline__ void locate_wave_add(uint64_t* bins, uint32_t nbins, uint32_t v, uint32_t n) {
  uint64_t live = __ballot(v != kLocateClean);
  while (live) {  // wave-uniform
    const int lead = __builtin_ctzll(live);
    const uint32_t lv = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), lead));
    const bool mine = v == lv;
    uint32_t sum = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) sum += static_cast<uint32_t>(__popcll(__ballot(mine && ((n >> b) & 1u)))) << b;
    if ((threadIdx.x & 63u) == static_cast<uint32_t>(lead) && sum) {
      if (PAIR && locate_is_pair(lv)) {
        atomicAdd(reinterpret_cast<unsigned long long*>(bins + ((lv >> 8) & 0xffu)),
                  static_cast<unsigned long long>(sum));
        atomicAdd(reinterpret_cast<unsigned long long*>(bins + (lv & 0xffu)),
                  static_cast<unsigned long long>(sum));
      } else {
        atomicAdd(reinterpret_cast<unsigned long long*>(bins + (lv == kLocateUnexplained ? nbins - 1 : lv)),
                  static_cast<unsigned long long>(sum));
      }
    }
    live &= ~__ballot(mine);
  }
}

}  // namespace dev
}  // namespace callfs

// decode-repair launches: built on the locate helpers above
#include "rs_repair.hpp"

namespace callfs {
namespace dev {

// The S % 16 tail of a locate launch: lds_tail with every row compared, and a mismatching
// byte classified and counted. Every thread of the waves that call it reaches the ballots.
// LOCATE 3 (a correct plan): a byte blamed on a shard is repaired there, with a byte store.
template <int RT, int LOCATE>
__device__ __forceinline__ void locate_tail(const ApplyArgs& a, const LocateArgs& x, cptr<const uint8_t*> in,
                                            cptr<uint8_t*> out, uint32_t stripe, uint32_t p,
                                            uint32_t lds0, uint32_t j, uint32_t out_stride) {
  constexpr bool PAIR = LOCATE == 2;
  constexpr int W = LdsAcc<RT>::W;
  const uint32_t nt = static_cast<uint32_t>(a.S - a.nvec * 16);
  uint32_t v = kLocateClean;
  if (j < nt) {
    const uint64_t b = a.nvec * 16 + j;
    typename LdsAcc<RT>::T t = lds_zero<RT>();
    for (int i0 = 0; i0 < a.K; i0 += tail_loads<RT>()) {
      uint32_t xb[tail_loads<RT>()];
      tail_bytes<RT>(in, b, i0, a.K, xb);
      for (int jj = 0; jj < tail_loads<RT>() && i0 + jj < a.K; ++jj) {
        const uint32_t base = lds0 + static_cast<uint32_t>(i0 + jj) * 32u * W;
        t = t ^ lds_lookup<RT>(base + (xb[jj] & 15u) * W) ^
            lds_lookup<RT>(base + 16u * W + (xb[jj] >> 4) * W);
      }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r)
      if (r < a.R) lds_xor_byte<RT>(t, r, out[r][b]);
    const uint8_t* pt = x.loc + static_cast<size_t>(p) * x.loc_stride;
    if constexpr (LOCATE == 3) {
      uint32_t pos = 0, val = 0;
      v = correct_column<RT>(t, a.R, a.K, x.gf, pt, pos, val);
      if (v < 256u) correct_shard(a, stripe, out_stride, pos)[b] ^= static_cast<uint8_t>(val);
    } else {
      v = locate_column<RT, PAIR>(t, a.R, a.K, x.gf, pt);
    }
  }
  if (__ballot(v != kLocateClean) == 0) return;  // wave-uniform
  if (v != kLocateClean) atomicOr(a.status + static_cast<size_t>(stripe) * a.status_stride, 1);
  locate_wave_add<PAIR>(x.counts + static_cast<size_t>(stripe) * x.nbins, x.nbins, v, v != kLocateClean ? 1u : 0u);
}

// One tile of one stripe: the body every mixed and ragged block runs once it knows its
// stripe, its tile within the stripe, the stripe's pattern p and (in `a`) the stripe's S,
// nvec and verify mask. Stages pattern p's tables into LDS, runs the S % 16 tail where
// a.tail_in_vec places it, then the input ring, lookups, stores and compares.
// SOME (the required plans' kernel): a.R is the stripe's own row count and
// out_stride the launch group's, the pitch of out_tab; rows at and past a.R have no pointer
// there and none is loaded.
// LOCATE (the locate plans' kernel, §5.12; with SOME): every row is compared. A lane whose 16
// bytes match in every row does what a verify lane does. A wave with a mismatching lane turns
// that lane's accumulators into the rows' syndromes (the stored bytes XORed in, read again),
// classifies its 16 byte columns with locate_classify and adds the columns per verdict into
// lx->counts, one atomic per verdict and wave (locate_wave_add); nothing block-wide follows the
// table prologue's barrier. LOCATE 2 (the pair plans' kernel, §5.12.1): the same with
// locate_classify2, in a loop over the 16 columns that is not unrolled, so that the kernel
// holds one copy of the rule (unrolled 16 times the 16-row instance spilled its accumulators).
// A lane that matches in every row runs none of it. LOCATE 3 (the correct plans' kernel, §5.13):
// the columns are classified with locate_correct, and a column blamed on a shard is repaired in
// that shard: the lane gathers its run's error values into one 16-byte vector and XORs it into
// the shard's vector. Counts and status words are a locate launch's.
template <int RT, class P, bool SOME = false, int LOCATE = 0>
__device__ __forceinline__ void mixed_tile(ApplyArgs& a, uint8_t* smem, uint32_t stripe, uint32_t tile,
                                           uint32_t p, uint32_t tab_stride, uint32_t out_stride = 0,
                                           const LocateArgs* lx = nullptr) {
  static_assert(LOCATE == 0 || SOME, "a locate launch reads the patterns' row counts");
  constexpr int BS = P::BS;
  constexpr int W = LdsAcc<RT>::W;
  static_assert(P::REALIGN == 0 && P::WIX == 0 && P::DMA == 0 && !P::NOMATH && !P::PERSIST && P::ORD == 0,
                "the plain ring forms in consecutive order only");
  using AccT = typename LdsAcc<RT>::T;
  const int K = a.K;
  const int R = a.R;
  const uint64_t v0 = static_cast<uint64_t>(tile) * BS + threadIdx.x;
  cptr<const uint8_t*> in = as_const(a.in_tab) + static_cast<size_t>(stripe) * K;
  cptr<uint8_t*> out = as_const(a.out_tab) + static_cast<size_t>(stripe) * (SOME ? out_stride : R);
  const bool active = v0 < a.nvec;
  auto ld = [&](int i) { return load16<P>(reinterpret_cast<const uint4*>(in[i]) + v0); };
  // The first input vectors go out before the table prologue: the prologue is a global
  // load that depends on pat[stripe], and a block has one tile to hide it behind.
  constexpr int NPRE = P::RING == 0 ? 2 : P::PD;
  uint4 xr[P::RING == 0 ? 3 : P::PD + 1];
#pragma unroll
  for (int s = 0; s < NPRE; ++s) xr[s] = make_uint4(0, 0, 0, 0);
  if (active) {
#pragma unroll
    for (int s = 0; s < NPRE; ++s)
      if (s < K) xr[s] = ld(s);
  }
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.ltabs + static_cast<size_t>(p) * tab_stride);
    uint4* dst = reinterpret_cast<uint4*>(smem);
    for (int j = threadIdx.x; j < K * 2 * W; j += BS) dst[j] = src[j];
  }
  __syncthreads();
  const uint32_t lds0 = static_cast<uint32_t>(
      reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)smem));
  if (a.tail_in_vec) {
    const uint32_t j = tail_lane<BS>(a.tail_in_vec, tile);
    if constexpr (LOCATE != 0) {
      if (j != ~0u) locate_tail<RT, LOCATE>(a, *lx, in, out, stripe, p, lds0, j, out_stride);
    } else {
      if (j != ~0u) lds_tail<RT>(a, in, out, stripe, lds0, j);
    }
  }
  if (!active) return;
  AccT acc[4][4];
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[w][j] = lds_zero<RT>();
  constexpr bool kVpf = P::VPF > 0 && RT <= 4;
  uint4 vpre[kVpf ? RT : 1];
#pragma unroll
  for (int r = 0; r < (kVpf ? RT : 1); ++r) vpre[r] = make_uint4(0, 0, 0, 0);

  if constexpr (P::RING == 0) {
    // ring of three shard vectors: shard i is consumed while i+1, i+2 load
    if (K < 2) xr[1] = xr[0];
    xr[2] = xr[0];
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
      if (i + 2 < K) xr[2] = ld(i + 2);
      if constexpr (kVpf) {
        if (i == (K > P::VPF ? K - P::VPF : 0)) {
#pragma unroll
          for (int r = 0; r < RT; ++r)
            if (r < R && ((a.verify_mask >> r) & 1u))
              vpre[r] = load16<P>(reinterpret_cast<const uint4*>(out[r]) + v0);
        }
      }
      lds_mac<RT, P::SDWA>(acc, xr[0], lds0 + static_cast<uint32_t>(i) * 32u * W);
      xr[0] = xr[1];
      xr[1] = xr[2];
    }
  } else {
    // PD+1 slots, shard i in slot i % NR; shard i+PD loads into the slot shard i-1 left
    constexpr int PD = P::PD, NR = P::PD + 1;
#pragma unroll 1
    for (int i0 = 0; i0 < K; i0 += NR) {
#pragma unroll
      for (int s = 0; s < NR; ++s) {
        const int i = i0 + s;
        if (i < K) {
          if (i + PD < K) xr[(s + PD) % NR] = ld(i + PD);
          lds_mac<RT, P::SDWA>(acc, xr[s], lds0 + static_cast<uint32_t>(i) * 32u * W);
        }
      }
    }
  }

  bool bad = false;
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    if (r >= R) continue;  // wave-uniform
    const uint4 o = make_uint4(lds_row<RT>(acc[0], r), lds_row<RT>(acc[1], r),
                               lds_row<RT>(acc[2], r), lds_row<RT>(acc[3], r));
    uint4* dst = reinterpret_cast<uint4*>(out[r]) + v0;
    if ((a.verify_mask >> r) & 1u) {
      uint4 y;
      if constexpr (kVpf) y = vpre[r];
      else y = load16<P>(dst);
      bad |= ((y.x ^ o.x) | (y.y ^ o.y) | (y.z ^ o.z) | (y.w ^ o.w)) != 0;
    } else {
      store16<P>(dst, o);
    }
  }
  if (bad) atomicOr(a.status + static_cast<size_t>(stripe) * a.status_stride, 1);
  if constexpr (LOCATE != 0) {
    if (__ballot(bad) == 0) return;  // wave-uniform: the lanes still here stay together below
    if (bad) {
      // acc's byte r holds row r's computed byte: XORing the stored one in leaves the syndrome
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r >= R) continue;
        uint4 y;
        if constexpr (kVpf) y = vpre[r];
        else y = load16<P>(reinterpret_cast<const uint4*>(out[r]) + v0);
        const uint32_t yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int j = 0; j < 4; ++j) lds_xor_byte<RT>(acc[w][j], r, (yw[w] >> (8 * j)) & 0xffu);
      }
    }
    const uint8_t* pt = lx->loc + static_cast<size_t>(p) * lx->loc_stride;
    uint64_t* bins = lx->counts + static_cast<size_t>(stripe) * lx->nbins;
    // a lane's columns almost always share one verdict: it keeps (verdict, columns) and the
    // wave adds a lane's run when its verdict changes, and every run at the end
    uint32_t run_v = kLocateClean, run_n = 0;
    auto note = [&](uint32_t v) {
      const bool flush = v != kLocateClean && run_n != 0 && v != run_v;
      if (__ballot(flush) != 0)
        locate_wave_add<LOCATE == 2>(bins, lx->nbins, flush ? run_v : kLocateClean, run_n);
      if (flush) run_n = 0;
      if (v != kLocateClean) {
        run_v = v;
        ++run_n;
      }
    };
    if constexpr (LOCATE == 3) {
      // the lane's correction of the shard its run blames, as the 16 bytes of its own vector:
      // XORed into the shard with one load and one store when the verdict changes and at the
      // end. No other lane touches these bytes.
      uint32_t cw[4] = {0, 0, 0, 0}, run_pos = 0;
      auto apply = [&]() {
        uint4* q = reinterpret_cast<uint4*>(correct_shard(a, stripe, out_stride, run_pos)) + v0;
        uint4 y = *q;
        y.x ^= cw[0];
        y.y ^= cw[1];
        y.z ^= cw[2];
        y.w ^= cw[3];
        *q = y;
#pragma unroll
        for (int w = 0; w < 4; ++w) cw[w] = 0;
      };
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t v = kLocateClean, pos = 0, val = 0;
          if (bad) v = correct_column<RT>(acc[w][j], R, K, lx->gf, pt, pos, val);
          if (v != kLocateClean && run_n != 0 && v != run_v && run_v < 256u) apply();
          note(v);
          if (v < 256u) {
            cw[w] |= val << (8 * j);
            run_pos = pos;
          }
        }
      if (run_n != 0 && run_v < 256u) apply();
    } else if constexpr (LOCATE == 2) {
      // one copy of the rule: the column index is wave-uniform and the column's syndromes are
      // picked out of the accumulators with selects, so the accumulators stay in registers
#pragma unroll 1
      for (int c = 0; c < 16; ++c) {
        uint32_t v = kLocateClean;
        if (bad) {
          AccT t = acc[0][0];
#pragma unroll
          for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (c == w * 4 + j) t = acc[w][j];
          v = locate_column<RT, true>(t, R, K, lx->gf, pt);
        }
        note(v);
      }
    } else {
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t v = kLocateClean;
          if (bad) v = locate_column<RT, false>(acc[w][j], R, K, lx->gf, pt);
          note(v);
        }
    }
    locate_wave_add<LOCATE == 2>(bins, lx->nbins, run_n ? run_v : kLocateClean, run_n);
  }
}

// An RT instance serves every R <= RT (rows >= R are computed and dropped). One tile of
// P::TILE_VECS vectors per block; block b works on tile a.t_base + b in consecutive order.
// (Blocks that work on 2..16 consecutive tiles of a stripe, to pay the table prologue once,
// measured 6-15 % slower: DESIGN.md §5.8.)
template <int RT, class P>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_apply_mixed(ApplyArgs a, MixedArgs x) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int TV = P::TILE_VECS;
  const uint32_t tps = static_cast<uint32_t>((a.nvec + TV - 1) / TV);
  const uint32_t ntiles = tps * static_cast<uint32_t>(a.batch);
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= ntiles) return;  // block-uniform
  const uint32_t stripe = t / tps, tile = t - stripe * tps;
  // the stripe's pattern: its tables and its compare mask (all wave-uniform)
  const uint32_t p = as_const(x.pat)[stripe];
  a.verify_mask = as_const(x.vmask)[p];
  mixed_tile<RT, P>(a, smem, stripe, tile, p, x.tab_stride);
}

// Ragged launches: every stripe its own shard size. The tile map gives the
// block its stripe with one scalar load; the stripe's first tile, its size and its pattern
// are three more that depend on it alone, and the verify mask one that depends on the
// pattern (all wave-uniform). From there the block is a mixed block of a plan whose S is
// the stripe's. A stripe shorter than 16 bytes is one tile with no vector: its block stages
// the tables, wave 0 computes the S % 16 tail from them, and every thread leaves.
template <int RT, class P>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_apply_ragged(ApplyArgs a, RaggedArgs x) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  static_assert(P::TILE_VECS == P::BS, "one vector per thread: the tile map counts 512-vector tiles");
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  a.S = as_const(x.size)[stripe];
  a.nvec = a.S / 16;
  a.verify_mask = as_const(x.vmask)[p];
  mixed_tile<RT, P>(a, smem, stripe, tile, p, x.tab_stride);
}

// Required launches: a ragged launch whose patterns have their own row
// counts. The tile map is the launch group's own and holds only the stripes with a row in
// the group; nrows[p] (wave-uniform, one more scalar load beside vmask[p]) is how many of
// pattern p's rows the group holds, 1..R. out_tab keeps the group's pitch R, and the block
// stores or compares rows [0, nrows[p]) alone -- in the vector body, the early compare
// loads and the S % 16 tail alike: the slots past them hold no pointer.
template <int RT, class P>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_apply_ragged_some(ApplyArgs a, RaggedSomeArgs xs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  static_assert(P::TILE_VECS == P::BS, "one vector per thread: the tile map counts 512-vector tiles");
  const RaggedArgs& x = xs.r;
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  a.S = as_const(x.size)[stripe];
  a.nvec = a.S / 16;
  a.verify_mask = as_const(x.vmask)[p];
  const uint32_t stride = static_cast<uint32_t>(a.R);
  a.R = static_cast<int>(as_const(xs.nrows)[p]);
  mixed_tile<RT, P, true>(a, smem, stripe, tile, p, x.tab_stride, stride);
}

// Locate launches: the required block setup, every row compared, and the
// mismatching byte columns classified and counted (mixed_tile LOCATE).
template <int RT, class P>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_apply_locate(ApplyArgs a, LocateArgs xl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  static_assert(P::TILE_VECS == P::BS, "one vector per thread: the tile map counts 512-vector tiles");
  const RaggedArgs& x = xl.r;
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  a.S = as_const(x.size)[stripe];
  a.nvec = a.S / 16;
  a.verify_mask = as_const(x.vmask)[p];
  const uint32_t stride = static_cast<uint32_t>(a.R);
  a.R = static_cast<int>(as_const(xl.nrows)[p]);
  mixed_tile<RT, P, true, 1>(a, smem, stripe, tile, p, x.tab_stride, stride, &xl);
}

// Pair locate launches: rs_apply_locate with locate_classify2 on the slow
// path. xl.gf and xl.loc are a pair plan's blocks (kLoc2GfBytes, locate_stride(K, 2)).
template <int RT, class P>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_apply_locate2(ApplyArgs a, LocateArgs xl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  static_assert(P::TILE_VECS == P::BS, "one vector per thread: the tile map counts 512-vector tiles");
  const RaggedArgs& x = xl.r;
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  a.S = as_const(x.size)[stripe];
  a.nvec = a.S / 16;
  a.verify_mask = as_const(x.vmask)[p];
  const uint32_t stride = static_cast<uint32_t>(a.R);
  a.R = static_cast<int>(as_const(xl.nrows)[p]);
  mixed_tile<RT, P, true, 2>(a, smem, stripe, tile, p, x.tab_stride, stride, &xl);
}

// Correct launches: rs_apply_locate that repairs what it blames. The shards
// in_tab and out_tab name are written through.
template <int RT, class P>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_apply_correct(ApplyArgs a, LocateArgs xl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  static_assert(P::TILE_VECS == P::BS, "one vector per thread: the tile map counts 512-vector tiles");
  const RaggedArgs& x = xl.r;
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  a.S = as_const(x.size)[stripe];
  a.nvec = a.S / 16;
  a.verify_mask = as_const(x.vmask)[p];
  const uint32_t stride = static_cast<uint32_t>(a.R);
  a.R = static_cast<int>(as_const(xl.nrows)[p]);
  mixed_tile<RT, P, true, 3>(a, smem, stripe, tile, p, x.tab_stride, stride, &xl);
}

// S < 16: one byte position per thread, 16 threads per stripe; the nibble tables are read
// from the arena in global memory (a launch of batch * S bytes has nothing to amortise an
// LDS prologue over). An RT instance (8 or 16: the entry width) serves every R <= RT.
template <int RT>
__global__ __launch_bounds__(kBlock) void rs_apply_mixed_bytes(ApplyArgs a, MixedArgs x) {
  constexpr int W = LdsAcc<RT>::W;
  using AccT = typename LdsAcc<RT>::T;
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t stripe = g >> 4, b = g & 15u;
  if (stripe >= static_cast<uint32_t>(a.batch) || b >= a.S) return;
  const uint32_t p = x.pat[stripe];
  const uint32_t vm = x.vmask[p];
  const uint8_t* tabs = a.ltabs + static_cast<size_t>(p) * x.tab_stride;
  const uint8_t* const* in = a.in_tab + static_cast<size_t>(stripe) * a.K;
  uint8_t* const* out = a.out_tab + static_cast<size_t>(stripe) * a.R;
  AccT t = lds_zero<RT>();
  for (int i = 0; i < a.K; ++i) {
    const uint32_t v = in[i][b];
    const uint8_t* ti = tabs + static_cast<size_t>(i) * 32u * W;
    t = t ^ *reinterpret_cast<const AccT*>(ti + (v & 15u) * W) ^
        *reinterpret_cast<const AccT*>(ti + 16u * W + (v >> 4) * W);
  }
  bool bad = false;
  for (int r = 0; r < a.R && r < RT; ++r) {
    const uint8_t v = static_cast<uint8_t>(lds_byte<RT>(t, r));
    if ((vm >> r) & 1u) bad |= out[r][b] != v;
    else out[r][b] = v;
  }
  if (bad) atomicOr(a.status + static_cast<size_t>(stripe) * a.status_stride, 1);
}

}  // namespace dev

namespace {

using MixedFn = void (*)(ApplyArgs, MixedArgs);

// [0]: R <= 4, [1]: R 5..8, [2]: R 9..16
const std::array<MixedFn, 3> kMixed = {&dev::rs_apply_mixed<4, dev::MixedPolicy<4>>,
                                       &dev::rs_apply_mixed<8, dev::MixedPolicy<8>>,
                                       &dev::rs_apply_mixed<16, dev::MixedPolicy<16>>};
const std::array<MixedFn, 2> kMixedBytes = {&dev::rs_apply_mixed_bytes<8>,
                                            &dev::rs_apply_mixed_bytes<16>};
using RaggedFn = void (*)(ApplyArgs, RaggedArgs);
const std::array<RaggedFn, 3> kRagged = {&dev::rs_apply_ragged<4, dev::MixedPolicy<4>>,
                                         &dev::rs_apply_ragged<8, dev::MixedPolicy<8>>,
                                         &dev::rs_apply_ragged<16, dev::MixedPolicy<16>>};
using RaggedSomeFn = void (*)(ApplyArgs, RaggedSomeArgs);
const std::array<RaggedSomeFn, 3> kRaggedSome = {&dev::rs_apply_ragged_some<4, dev::MixedPolicy<4>>,
                                                 &dev::rs_apply_ragged_some<8, dev::MixedPolicy<8>>,
                                                 &dev::rs_apply_ragged_some<16, dev::MixedPolicy<16>>};
using LocateFn = void (*)(ApplyArgs, LocateArgs);
const std::array<LocateFn, 3> kLocate = {&dev::rs_apply_locate<4, dev::MixedPolicy<4>>,
                                         &dev::rs_apply_locate<8, dev::MixedPolicy<8>>,
                                         &dev::rs_apply_locate<16, dev::MixedPolicy<16>>};
const std::array<LocateFn, 3> kLocate2 = {&dev::rs_apply_locate2<4, dev::MixedPolicy<4>>,
                                          &dev::rs_apply_locate2<8, dev::MixedPolicy<8>>,
                                          &dev::rs_apply_locate2<16, dev::MixedPolicy<16>>};
const std::array<LocateFn, 3> kCorrect = {&dev::rs_apply_correct<4, dev::MixedPolicy<4>>,
                                          &dev::rs_apply_correct<8, dev::MixedPolicy<8>>,
                                          &dev::rs_apply_correct<16, dev::MixedPolicy<16>>};
static_assert(dev::MixedPolicy<4>::BS == 512 && dev::MixedPolicy<8>::BS == 512 &&
                  dev::MixedPolicy<16>::BS == 512 && dev::MixedPolicy<4>::TILE_VECS == 512 &&
                  dev::MixedPolicy<8>::TILE_VECS == 512 && dev::MixedPolicy<16>::TILE_VECS == 512,
              "one grid shape for every mixed instance");
constexpr uint32_t kMixedBlock = 512, kMixedTileVecs = 512;
static_assert(kRaggedLaunchTileVecs == kMixedTileVecs, "the tile map counts the instances' tiles");

// Update launches (rs_update.hpp): [pair][0: R <= 4, 1: R 5..8, 2: R 9..16]
using UpdateFn = void (*)(ApplyArgs, UpdateArgs);
template <int RT, bool PAIR>
constexpr UpdateFn kUpdateInstance = &dev::rs_update_ragged<RT, dev::UpdatePolicyFor<RT, PAIR>, PAIR>;
const std::array<std::array<UpdateFn, 3>, 2> kUpdate = {{
    {kUpdateInstance<4, false>, kUpdateInstance<8, false>, kUpdateInstance<16, false>},
    {kUpdateInstance<4, true>, kUpdateInstance<8, true>, kUpdateInstance<16, true>}}};

// Decode-idx launches (rs_merge.hpp): [store][0: R <= 4, 1: R 5..8, 2: R 9..16]
using MergeFn = void (*)(ApplyArgs, MergeArgs);
template <int RT, bool STORE>
constexpr MergeFn kMergeInstance = &dev::rs_merge_ragged<RT, dev::UpdatePolicyFor<RT, false>, STORE>;
const std::array<std::array<MergeFn, 3>, 2> kMerge = {{
    {kMergeInstance<4, false>, kMergeInstance<8, false>, kMergeInstance<16, false>},
    {kMergeInstance<4, true>, kMergeInstance<8, true>, kMergeInstance<16, true>}}};

// Final decode-check launches (rs_check.hpp): [store][0: R <= 4, 1: R 5..8, 2: R 9..16]
using CheckFn = void (*)(ApplyArgs, CheckArgs);
template <int RT, bool STORE>
constexpr CheckFn kCheckInstance = &dev::rs_check_ragged<RT, dev::UpdatePolicyFor<RT, false>, STORE>;
const std::array<std::array<CheckFn, 3>, 2> kCheck = {{
    {kCheckInstance<4, false>, kCheckInstance<8, false>, kCheckInstance<16, false>},
    {kCheckInstance<4, true>, kCheckInstance<8, true>, kCheckInstance<16, true>}}};

// Decode-repair launches (rs_repair.hpp): [store][0: R <= 4, 1: R 5..8, 2: R 9..16]
using RepairFn = void (*)(ApplyArgs, RepairArgs);
template <int RT, bool STORE>
constexpr RepairFn kRepairInstance = &dev::rs_repair_ragged<RT, dev::UpdatePolicyFor<RT, false>, STORE>;
const std::array<std::array<RepairFn, 3>, 2> kRepair = {{
    {kRepairInstance<4, false>, kRepairInstance<8, false>, kRepairInstance<16, false>},
    {kRepairInstance<4, true>, kRepairInstance<8, true>, kRepairInstance<16, true>}}};

// Feed launches (rs_feed.hpp): [store][0: R <= 4, 1: R 5..8, 2: R 9..16]
template <int RT>
using FeedFn = void (*)(ApplyArgs, FeedRows<RT>);
template <int RT>
constexpr std::array<FeedFn<RT>, 2> kFeed = {&dev::rs_feed<RT, false>, &dev::rs_feed<RT, true>};

template <int RT>
void dispatch_feed(const ApplyArgs& a, const FeedArgs& x, bool store, uint32_t grid, hipStream_t stream,
                   const LaunchEvents& ev) {
  FeedRows<RT> rows{};
  rows.src = x.src;
  if constexpr (RT <= 8)
    for (int r = 0; r < a.R; ++r) rows.row[r] = x.rows[r];
  dispatch(kFeed<RT>[store ? 1 : 0], dim3(grid), dim3(dev::kFeedBlock), 0, stream, ev, true, true, a, rows);
}

// Absorb launches (rs_absorb.hpp)
template <int RT>
void dispatch_absorb(const ApplyArgs& a, const AbsorbArgs& x, hipStream_t stream, const LaunchEvents& ev) {
  AbsorbRows<RT> rows{};
  rows.src = x.src;
  rows.off = x.off;
  for (int q = 0; q < kAbsorbMaxIntervals; ++q) {
    rows.iv[q] = x.plan.iv[q];
    rows.end[q] = x.plan.end[q];
  }
  if constexpr (RT <= 8)
    for (int r = 0; r < a.R; ++r) rows.row[r] = x.rows[r];
  dispatch(&dev::rs_absorb<RT>, dim3(x.plan.grid()), dim3(dev::kFeedBlock), 0, stream, ev, true, true, a, rows);
}

// 16-row groups with more than 64 KiB of tables (k > 128) need the dynamic-LDS opt-in, a
// per-device attribute (dispatch.hpp DeviceOnce), keyed by the 16-row instance it is set on
enum class WideLds { kMixed, kRagged, kRaggedSome, kUpdate, kUpdatePair, kLocate, kLocate2, kCorrect,
                     kMerge, kMergeStore, kCheck, kCheckStore, kRepair, kRepairStore };
DeviceOnce g_mixed_wide_lds;

// The vector launch every kind shares: the dynamic-LDS opt-in, then `grid` tiles in equal
// consecutive slices of `streams` shard streams, as launch_apply cuts them. A slice boundary
// may fall inside a stripe (tiles are numbered over the whole grid).
template <class X>
hipError_t launch_tiles(void (*fn)(ApplyArgs, X), WideLds once_key, uint32_t grid, ApplyArgs& a,
                        const X& x, int streams, hipStream_t stream, const LaunchEvents& ev) {
  const size_t lds = dev::lds_bytes(a.K, a.R > 8 ? 16 : 8);
  if (lds > (64u << 10)) {
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess) return hipErrorInvalidDevice;
    g_mixed_wide_lds.run(device, static_cast<int>(once_key), [fn] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
    });
  }
  launch_slices(grid, launch_slice_tiles(streams), a, [&](uint32_t blocks, bool first, bool last) {
    dispatch(fn, dim3(blocks), dim3(kMixedBlock), lds, stream, ev, first, last, a, x);
  });
  return hipGetLastError();
}

// What every launch over a tile map (X: RaggedArgs or UpdateArgs) checks of its arguments: the
// launch group's shape, the pointer tables and the map.
template <class X>
bool tile_map_ok(const ApplyArgs& a, const X& x) {
  return a.R >= 1 && a.R <= kMaxRowsPerLaunch && a.K >= 1 && a.K <= kMaxK && a.batch >= 1 && a.ltabs &&
         x.pat && x.size && x.tile0 && a.in_tab && a.out_tab && x.ntiles <= 0x7fffffffu &&
         (x.ntiles == 0 || x.tile_stripe);
}

}  // namespace

hipError_t launch_mixed(ApplyArgs a, const MixedArgs& x, hipStream_t stream, LaunchEvents ev) {
  if (a.R < 1 || a.R > kMaxRowsPerLaunch || a.K < 1 || a.K > kMaxK || a.batch < 1 || !a.ltabs ||
      !x.pat || !x.vmask || !a.in_tab || !a.out_tab || !a.status)
    return hipErrorInvalidValue;
  if (a.S == 0) return hipSuccess;
  a.t_base = 0;
  a.nvec = a.S / 16;
  if (a.nvec == 0) {
    const uint64_t threads = static_cast<uint64_t>(a.batch) * 16u;
    dispatch(kMixedBytes[a.R > 8 ? 1 : 0], dim3(static_cast<unsigned>((threads + dev::kBlock - 1) / dev::kBlock)),
             dim3(dev::kBlock), 0, stream, ev, true, true, a, x);
    return hipGetLastError();
  }
  // the S % 16 tail: wave 0 of each stripe's first tile (rs_apply.hpp tail_lane)
  a.tail_in_vec = a.nvec * 16 < a.S ? 1u : 0u;
  const uint64_t tps = (a.nvec + kMixedTileVecs - 1) / kMixedTileVecs;
  const uint64_t ntiles = tps * static_cast<uint64_t>(a.batch);
  if (ntiles > 0x7fffffffull) return hipErrorInvalidValue;
  return launch_tiles(kMixed[a.R > 8 ? 2 : a.R > 4 ? 1 : 0], WideLds::kMixed, static_cast<uint32_t>(ntiles), a, x,
                      a.K + a.R, stream, ev);
}

hipError_t launch_ragged(ApplyArgs a, const RaggedArgs& x, const uint32_t* nrows, bool any_tail,
                         hipStream_t stream, LaunchEvents ev) {
  if (!tile_map_ok(a, x) || !x.vmask || !a.status ||
      (!nrows && x.ntiles < static_cast<uint32_t>(a.batch)))  // without row counts every stripe has a tile
    return hipErrorInvalidValue;
  if (x.ntiles == 0) return hipSuccess;  // no stripe has a row in this launch group
  a.t_base = 0;
  a.S = a.nvec = 0;  // per stripe, read by the kernel
  // the S % 16 tails: wave 0 of each stripe's first tile (rs_apply.hpp tail_lane); stripes
  // with no tail leave lds_tail at once
  a.tail_in_vec = any_tail ? 1u : 0u;
  const int inst = a.R > 8 ? 2 : a.R > 4 ? 1 : 0;
  return nrows ? launch_tiles(kRaggedSome[inst], WideLds::kRaggedSome, x.ntiles, a, RaggedSomeArgs{x, nrows},
                              a.K + a.R, stream, ev)
               : launch_tiles(kRagged[inst], WideLds::kRagged, x.ntiles, a, x, a.K + a.R, stream, ev);
}

namespace {

// launch_locate and launch_correct: `fns` with the dynamic-LDS key `once_key`
hipError_t launch_locate_kind(const std::array<LocateFn, 3>& fns, WideLds once_key, ApplyArgs a, const LocateArgs& x,
                              bool any_tail, hipStream_t stream, LaunchEvents ev, int max_errors) {
  const RaggedArgs& r = x.r;
  if (!tile_map_ok(a, r) || !r.vmask || !a.status || !x.nrows || !x.gf || !x.loc || !x.counts ||
      max_errors < 1 || max_errors > 2 || x.loc_stride != locate_stride(a.K, max_errors) || x.nbins < 2)
    return hipErrorInvalidValue;
  if (r.ntiles == 0) return hipSuccess;  // no stripe has a row
  a.t_base = 0;
  a.S = a.nvec = 0;  // per stripe, read by the kernel
  a.tail_in_vec = any_tail ? 1u : 0u;  // wave 0 of each stripe's first tile
  return launch_tiles(fns[a.R > 8 ? 2 : a.R > 4 ? 1 : 0], once_key, r.ntiles, a, x, a.K + a.R, stream, ev);
}

}  // namespace

hipError_t launch_locate(ApplyArgs a, const LocateArgs& x, bool any_tail, hipStream_t stream,
                         LaunchEvents ev, int max_errors) {
  return max_errors == 2 ? launch_locate_kind(kLocate2, WideLds::kLocate2, a, x, any_tail, stream, ev, 2)
                         : launch_locate_kind(kLocate, WideLds::kLocate, a, x, any_tail, stream, ev, max_errors);
}

hipError_t launch_correct(ApplyArgs a, const LocateArgs& x, bool any_tail, hipStream_t stream,
                          LaunchEvents ev) {
  return launch_locate_kind(kCorrect, WideLds::kCorrect, a, x, any_tail, stream, ev, 1);
}

hipError_t launch_update(ApplyArgs a, const UpdateArgs& x, bool pair, bool any_tail,
                         hipStream_t stream, LaunchEvents ev) {
  if (!tile_map_ok(a, x) || !x.nsrc || x.in_stride != static_cast<uint32_t>(a.K) * (pair ? 2u : 1u))
    return hipErrorInvalidValue;
  if (x.ntiles == 0) return hipSuccess;  // no stripe has a changed shard
  a.t_base = 0;
  a.S = a.nvec = 0;  // per stripe, read by the kernel
  a.verify_mask = 0;
  a.tail_in_vec = any_tail ? 1u : 0u;  // wave 0 of each stripe's first tile
  // per tile: the sources (twice for pairs), and every row read and written
  return launch_tiles(kUpdate[pair ? 1 : 0][a.R > 8 ? 2 : a.R > 4 ? 1 : 0],
                      pair ? WideLds::kUpdatePair : WideLds::kUpdate, x.ntiles, a, x,
                      a.K * (pair ? 2 : 1) + 2 * a.R, stream, ev);
}

hipError_t launch_decode_idx(ApplyArgs a, const MergeArgs& x, bool store, bool any_tail,
                             hipStream_t stream, LaunchEvents ev) {
  if (!tile_map_ok(a, x.u) || !x.u.nsrc || !x.nrows || x.u.in_stride != static_cast<uint32_t>(a.K))
    return hipErrorInvalidValue;
  if (x.u.ntiles == 0) return hipSuccess;  // no stripe has both a delivered and a wanted shard
  a.t_base = 0;
  a.S = a.nvec = 0;  // per stripe, read by the kernel
  a.verify_mask = 0;
  a.tail_in_vec = any_tail ? 1u : 0u;  // wave 0 of each stripe's first tile
  // per tile: the sources, and every row written (merge: read as well)
  return launch_tiles(kMerge[store ? 1 : 0][a.R > 8 ? 2 : a.R > 4 ? 1 : 0],
                      store ? WideLds::kMergeStore : WideLds::kMerge, x.u.ntiles, a, x,
                      a.K + (store ? 1 : 2) * a.R, stream, ev);
}

hipError_t launch_feed(const FeedArgs& x, bool store, hipStream_t stream, LaunchEvents ev) {
  if (x.R < 0 || x.R > kMaxRowsPerLaunch || !x.src || !x.tabs || !x.row_tab || !x.rows || x.S == 0)
    return hipErrorInvalidValue;
  if (x.R == 0) return hipSuccess;  // no row to feed
  const uint64_t grid = (x.S + kFeedTileBytes - 1) / kFeedTileBytes;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  ApplyArgs a{};
  a.out_tab = x.row_tab;
  a.tabs = x.tabs;
  a.S = x.S;
  a.nvec = x.S / 16;
  a.K = 1;
  a.R = x.R;
  a.batch = 1;
  if (x.R > 8) dispatch_feed<16>(a, x, store, static_cast<uint32_t>(grid), stream, ev);
  else if (x.R > 4) dispatch_feed<8>(a, x, store, static_cast<uint32_t>(grid), stream, ev);
  else dispatch_feed<4>(a, x, store, static_cast<uint32_t>(grid), stream, ev);
  return hipGetLastError();
}

hipError_t launch_absorb(const AbsorbArgs& x, hipStream_t stream, LaunchEvents ev) {
  if (x.R < 1 || x.R > kMaxRowsPerLaunch || x.K < 1 || x.K > kMaxK || !x.src || !x.tabs || !x.row_tab || !x.rows ||
      x.S == 0 || x.len == 0)
    return hipErrorInvalidValue;
  // the plan is the range's: every interval inside [0, S) x [0, K) with its bytes inside the range,
  // and the block counts those of its columns
  const AbsorbPlan& p = x.plan;
  if (p.n < 1 || p.n > kAbsorbMaxIntervals) return hipErrorInvalidValue;
  uint64_t blocks = 0;
  for (int q = 0; q < kAbsorbMaxIntervals; ++q) {
    if (q < p.n) {
      const AbsorbInterval& v = p.iv[q];
      if (v.col0 >= v.col1 || v.col1 > x.S || v.shard0 < 0 || v.shard0 > v.shard1 || v.shard1 >= x.K ||
          static_cast<uint64_t>(v.shard0) * x.S + v.col0 < x.off ||
          static_cast<uint64_t>(v.shard1) * x.S + v.col1 > x.off + x.len)
        return hipErrorInvalidValue;
      blocks += (v.col1 - v.col0 + kFeedTileBytes - 1) / kFeedTileBytes;
    }
    if (blocks > 0x7fffffffull || p.end[q] != blocks) return hipErrorInvalidValue;
  }
  ApplyArgs a{};
  a.out_tab = x.row_tab;
  a.tabs = x.tabs;
  a.S = x.S;
  a.nvec = x.S / 16;
  a.K = x.K;
  a.R = x.R;
  a.batch = 1;
  if (x.R > 8) dispatch_absorb<16>(a, x, stream, ev);
  else if (x.R > 4) dispatch_absorb<8>(a, x, stream, ev);
  else dispatch_absorb<4>(a, x, stream, ev);
  return hipGetLastError();
}

hipError_t launch_decode_check(ApplyArgs a, const CheckArgs& x, bool store, bool any_tail,
                               hipStream_t stream, LaunchEvents ev) {
  const UpdateArgs& u = x.m.u;
  // tile_map_ok, but for a.K: no pattern of a final launch need have a source
  if (a.R < 1 || a.R > kMaxRowsPerLaunch || a.K < 0 || a.K > kMaxK || a.batch < 1 || !a.ltabs || !u.pat ||
      !u.size || !u.tile0 || !a.in_tab || !a.out_tab || u.ntiles > 0x7fffffffu || (u.ntiles != 0 && !u.tile_stripe) ||
      !u.nsrc || !x.m.nrows || !x.cmask || !a.status || u.in_stride != static_cast<uint32_t>(a.K))
    return hipErrorInvalidValue;
  if (u.ntiles == 0) return hipSuccess;  // no stripe has a row
  a.t_base = 0;
  a.S = a.nvec = 0;  // per stripe, read by the kernel
  a.verify_mask = 0;
  a.tail_in_vec = any_tail ? 1u : 0u;  // wave 0 of each stripe's first tile
  // per tile: the sources, and every row read (merge) or written (store) at least once
  return launch_tiles(kCheck[store ? 1 : 0][a.R > 8 ? 2 : a.R > 4 ? 1 : 0],
                      store ? WideLds::kCheckStore : WideLds::kCheck, u.ntiles, a, x, a.K + a.R, stream, ev);
}

hipError_t launch_decode_repair(ApplyArgs a, const RepairArgs& x, bool store, bool any_tail,
                                hipStream_t stream, LaunchEvents ev) {
  const UpdateArgs& u = x.c.m.u;
  // launch_decode_check's test, and what the slow path reads
  if (a.R < 1 || a.R > kMaxRowsPerLaunch || a.K < 0 || a.K > kMaxK || a.batch < 1 || !a.ltabs || !u.pat ||
      !u.size || !u.tile0 || !a.in_tab || !a.out_tab || u.ntiles > 0x7fffffffu || (u.ntiles != 0 && !u.tile_stripe) ||
      !u.nsrc || !x.c.m.nrows || !x.c.cmask || !a.status || u.in_stride != static_cast<uint32_t>(a.K) || !x.gf ||
      !x.loc || !x.counts || !x.fix || x.k < 1 || x.k > kMaxK || x.loc_stride != locate_stride(x.k) || x.nbins < 2)
    return hipErrorInvalidValue;
  if (u.ntiles == 0) return hipSuccess;  // no stripe has a row
  a.t_base = 0;
  a.S = a.nvec = 0;  // per stripe, read by the kernel
  a.verify_mask = 0;
  a.tail_in_vec = any_tail ? 1u : 0u;  // wave 0 of each stripe's first tile
  // per tile: the sources, and every row read (merge) or written (store) at least once
  return launch_tiles(kRepair[store ? 1 : 0][a.R > 8 ? 2 : a.R > 4 ? 1 : 0],
                      store ? WideLds::kRepairStore : WideLds::kRepair, u.ntiles, a, x, a.K + a.R, stream, ev);
}

}  // namespace callfs
