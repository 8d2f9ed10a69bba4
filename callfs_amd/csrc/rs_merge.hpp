// Decode-idx launches: upstream DecodeIdx on the device. The single-source
// form of rs_update_ragged (rs_update.hpp: the ragged block setup from the tile map, the first
// source loads ahead of the table prologue, the same ring, lds_mac, non-temporal accesses and
// plain unaligned 16-byte accesses) with two additions: the row count is the pattern's own,
// R = nrows[p], read beside nsrc[p], with the destination table pitched at the launch group's
// row count and rows >= R computed and dropped, never loaded or stored; and STORE, which stores
// every row as computed and loads no destination byte anywhere, in the vector path or in the
// S % 16 tail. No verify mask, no status word, no atomics. Included by rs_mixed.hip alone.
#pragma once

#include "rs_update.hpp"

namespace callfs {
namespace dev {

// update_tail with the pattern's row count, and its store form: byte b = 16 * nvec + j of every
// row r < R becomes the row's product over the C sources, XORed into out[r][b] unless STORE.
template <int RT, bool STORE>
__device__ __forceinline__ void merge_tail(uint64_t S, uint64_t nvec, int C, int R,
                                           cptr<const uint8_t*> in, cptr<uint8_t*> out,
                                           uint32_t lds0, uint32_t j) {
  constexpr int W = LdsAcc<RT>::W;
  const uint32_t nt = static_cast<uint32_t>(S - nvec * 16);
  if (j >= nt) return;
  const uint64_t b = nvec * 16 + j;
  typename LdsAcc<RT>::T t = lds_zero<RT>();
  for (int i0 = 0; i0 < C; i0 += 4) {
    uint32_t x[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) x[s] = i0 + s < C ? in[i0 + s][b] : 0u;
    for (int s = 0; s < 4 && i0 + s < C; ++s) {
      const uint32_t base = lds0 + static_cast<uint32_t>(i0 + s) * 32u * W;
      t = t ^ lds_lookup<RT>(base + (x[s] & 15u) * W) ^ lds_lookup<RT>(base + 16u * W + (x[s] >> 4) * W);
    }
  }
  for (int r = 0; r < R && r < RT; ++r) {
    if constexpr (STORE) out[r][b] = static_cast<uint8_t>(lds_byte<RT>(t, r));
    else out[r][b] = static_cast<uint8_t>(out[r][b] ^ lds_byte<RT>(t, r));
  }
}

// An RT instance serves every launch group of up to RT rows. One tile of 512 vectors per block;
// block b works on tile a.t_base + b in consecutive order. The tile map is the plan's, shared by
// its launch groups: a stripe whose pattern has no row in this group (nrows[p] == 0: at most 16
// wanted rows, in a plan where another stripe has more) leaves before its first load.
template <int RT, class P, bool STORE>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_merge_ragged(ApplyArgs a, MergeArgs xm) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int BS = P::BS;
  constexpr int W = LdsAcc<RT>::W;
  constexpr int PD = P::PD, NR = P::PD + 1;
  static_assert(P::TILE_VECS == BS, "one vector per thread: the tile map counts 512-vector tiles");
  using AccT = typename LdsAcc<RT>::T;
  const UpdateArgs& x = xm.u;
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  // the stripe, its tile, its size, its pattern and the pattern's source and row counts: all
  // wave-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  const uint64_t S = as_const(x.size)[stripe];
  const uint64_t nvec = S / 16;
  const int C = static_cast<int>(as_const(x.nsrc)[p]);
  const int R = static_cast<int>(as_const(xm.nrows)[p]);
  if (R == 0) return;  // block-uniform
  const uint64_t v0 = static_cast<uint64_t>(tile) * BS + threadIdx.x;
  cptr<const uint8_t*> in = as_const(a.in_tab) + static_cast<size_t>(stripe) * x.in_stride;
  cptr<uint8_t*> out = as_const(a.out_tab) + static_cast<size_t>(stripe) * a.R;
  const bool active = v0 < nvec;
  auto ld = [&](int i) { return load16<P>(reinterpret_cast<const uint4*>(in[i]) + v0); };
  // The first sources go out before the table prologue, as in rs_update_ragged.
  uint4 xr[NR];
#pragma unroll
  for (int s = 0; s < NR; ++s) xr[s] = make_uint4(0, 0, 0, 0);
  if (active) {
#pragma unroll
    for (int s = 0; s < PD; ++s)
      if (s < C) xr[s] = ld(s);
  }
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.ltabs + static_cast<size_t>(p) * x.tab_stride);
    uint4* dst = reinterpret_cast<uint4*>(smem);
    for (int j = threadIdx.x; j < C * 2 * W; j += BS) dst[j] = src[j];
  }
  __syncthreads();
  const uint32_t lds0 = static_cast<uint32_t>(
      reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)smem));
  if (a.tail_in_vec) {
    const uint32_t j = tail_lane<BS>(a.tail_in_vec, tile);
    if (j != ~0u) merge_tail<RT, STORE>(S, nvec, C, R, in, out, lds0, j);
  }
  if (!active) return;
  AccT acc[4][4];
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[w][j] = lds_zero<RT>();
  // the early destination loads of RT 4 (UpdatePolicy::VPF): a merge instance's alone
  constexpr bool kVpf = P::VPF > 0 && !STORE;
  static_assert(!kVpf || RT <= 4, "early destination loads: RT <= 4 only");
  uint4 vpre[kVpf ? RT : 1];
  if constexpr (kVpf) {
#pragma unroll
    for (int r = 0; r < RT; ++r) vpre[r] = make_uint4(0, 0, 0, 0);
  }
  const int vat = C > P::VPF ? C - P::VPF : 0;

  // PD + 1 slots, source i in slot i % NR; source i + PD loads into the slot source i - 1 left
#pragma unroll 1
  for (int i0 = 0; i0 < C; i0 += NR) {
#pragma unroll
    for (int s = 0; s < NR; ++s) {
      const int i = i0 + s;
      if (i < C) {
        if (i + PD < C) xr[(s + PD) % NR] = ld(i + PD);
        if constexpr (kVpf) {
          if (i == vat) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
              if (r < R) vpre[r] = load16<P>(reinterpret_cast<const uint4*>(out[r]) + v0);
          }
        }
        lds_mac<RT, P::SDWA>(acc, xr[s], lds0 + static_cast<uint32_t>(i) * 32u * W);
      }
    }
  }

  if constexpr (STORE) {
    // every row as computed: nothing of the destination is read
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      if (r >= R) continue;  // wave-uniform
      store16<P>(reinterpret_cast<uint4*>(out[r]) + v0,
                 make_uint4(lds_row<RT>(acc[0], r), lds_row<RT>(acc[1], r), lds_row<RT>(acc[2], r),
                            lds_row<RT>(acc[3], r)));
    }
  } else if constexpr (kVpf) {
    // every row: the destination's 16 bytes XOR the row, stored where they were loaded
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      if (r >= R) continue;  // wave-uniform
      const uint4 y = vpre[r];
      store16<P>(reinterpret_cast<uint4*>(out[r]) + v0,
                 make_uint4(y.x ^ lds_row<RT>(acc[0], r), y.y ^ lds_row<RT>(acc[1], r),
                            y.z ^ lds_row<RT>(acc[2], r), y.w ^ lds_row<RT>(acc[3], r)));
    }
  } else {
    // four rows' loads in flight, then their four stores (a store may alias a later load for
    // all the compiler knows, so it keeps the order written here)
#pragma unroll
    for (int r0 = 0; r0 < RT; r0 += 4) {
      if (r0 >= R) continue;  // wave-uniform
      uint4 y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        y[q] = make_uint4(0, 0, 0, 0);
        if (r0 + q < R) y[q] = load16<P>(reinterpret_cast<const uint4*>(out[r0 + q]) + v0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + q;
        if (r >= R) continue;
        store16<P>(reinterpret_cast<uint4*>(out[r]) + v0,
                   make_uint4(y[q].x ^ lds_row<RT>(acc[0], r), y[q].y ^ lds_row<RT>(acc[1], r),
                              y[q].z ^ lds_row<RT>(acc[2], r), y[q].w ^ lds_row<RT>(acc[3], r)));
      }
    }
  }
}

}  // namespace dev
}  // namespace callfs
