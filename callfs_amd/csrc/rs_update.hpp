// Update launches: upstream Update and EncodeIdx on the device. A ragged
// block (§5.9: the tile map gives the block its stripe, tile, size and pattern) with four
// differences: it stages the tables of its pattern's nsrc[p] changed shards alone; a source is
// a pair (old, new) whose XOR is formed in registers, so a changed shard costs one lookup pass,
// not two (PAIR), or one shard (EncodeIdx); every row r < R is read from its destination and
// stored back XORed with the row's product, from the same lane to the same address; and the
// S % 16 tail accumulates too, byte by byte, in wave 0 of the stripe's first tile. No verify
// mask, no status word, no atomics. Included by rs_mixed.hip alone.
#pragma once

#include "rs_apply.hpp"

namespace callfs {
namespace dev {

// PD sources ahead in a ring of PD + 1 slots (a slot of a PAIR kernel holds two vectors);
// SDWA table addresses for the 16-byte entries, as MixedPolicy16; VPF > 0: the R destination
// loads are issued VPF sources before the end of the source loop (RT <= 4, as the mixed
// kernels' compared rows), else after it in groups of four rows. (At RT 4 the early loads cost
// the pair instance two waves per SIMD, 76 VGPRs against 60, and are still the faster form:
// RS(10,4) 256 x 1 MiB with one changed shard 427 us against 456, with five 828 against 824;
// DESIGN.md §5.11.) Loads and stores
// non-temporal, 512 threads and one vector per thread, as every mixed instance.
template <int PD_, bool SDWA_, int VPF_>
struct UpdatePolicy {
  static constexpr int PD = PD_;
  static constexpr bool SDWA = SDWA_;
  static constexpr int VPF = VPF_;
  static constexpr int BS = 512;
  static constexpr int TILE_VECS = 512;
  static constexpr int WPE = 2;
  static constexpr bool NT_LOAD = true;
  static constexpr bool NT_STORE = true;
};
// The ring keeps as many sources ahead as the mixed policies do: 2 for RT <= 8, 4 for RT 16 --
// but for the RT 16 pair instance, whose five pair slots took it to 142 VGPRs and 3 waves per
// SIMD (one 512-thread block per CU instead of two): two pairs ahead keep it under 128.
template <int RT, bool PAIR>
using UpdatePolicyFor = typename std::conditional<
    (RT > 8), UpdatePolicy<(PAIR ? 2 : 4), true, 0>,
    typename std::conditional<(RT > 4), UpdatePolicy<2, false, 0>, UpdatePolicy<2, false, 4>>::type>::type;

template <bool PAIR>
struct UpdateSrc {
  uint4 a, b;  // old, new
};
template <>
struct UpdateSrc<false> {
  uint4 a;
};

template <bool PAIR>
__device__ __forceinline__ uint4 update_delta(const UpdateSrc<PAIR>& s) {
  if constexpr (PAIR) return make_uint4(s.a.x ^ s.b.x, s.a.y ^ s.b.y, s.a.z ^ s.b.z, s.a.w ^ s.b.w);
  else return s.a;
}

// The accumulating form of lds_tail: byte b = 16 * nvec + j of every row r < R becomes
// out[r][b] ^ the row's product over the C sources; loads four sources at a time.
template <int RT, bool PAIR>
__device__ __forceinline__ void update_tail(uint64_t S, uint64_t nvec, int C, int R,
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
    for (int s = 0; s < 4; ++s) {
      const int i = i0 + s;
      if (i >= C) x[s] = 0u;
      else if constexpr (PAIR) x[s] = static_cast<uint32_t>(in[2 * i][b]) ^ in[2 * i + 1][b];
      else x[s] = in[i][b];
    }
    for (int s = 0; s < 4 && i0 + s < C; ++s) {
      const uint32_t base = lds0 + static_cast<uint32_t>(i0 + s) * 32u * W;
      t = t ^ lds_lookup<RT>(base + (x[s] & 15u) * W) ^ lds_lookup<RT>(base + 16u * W + (x[s] >> 4) * W);
    }
  }
  for (int r = 0; r < R && r < RT; ++r)
    out[r][b] = static_cast<uint8_t>(out[r][b] ^ lds_byte<RT>(t, r));
}

// An RT instance serves every R <= RT (rows >= R are computed and dropped). One tile of 512
// vectors per block; block b works on tile a.t_base + b in consecutive order.
template <int RT, class P, bool PAIR>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_update_ragged(ApplyArgs a, UpdateArgs x) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int BS = P::BS;
  constexpr int W = LdsAcc<RT>::W;
  constexpr int PD = P::PD, NR = P::PD + 1;
  static_assert(P::TILE_VECS == BS, "one vector per thread: the tile map counts 512-vector tiles");
  using AccT = typename LdsAcc<RT>::T;
  using Src = UpdateSrc<PAIR>;
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  // the stripe, its tile, its size, its pattern and the pattern's source count: all wave-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  const uint64_t S = as_const(x.size)[stripe];
  const uint64_t nvec = S / 16;
  const int C = static_cast<int>(as_const(x.nsrc)[p]);
  const int R = a.R;
  const uint64_t v0 = static_cast<uint64_t>(tile) * BS + threadIdx.x;
  cptr<const uint8_t*> in = as_const(a.in_tab) + static_cast<size_t>(stripe) * x.in_stride;
  cptr<uint8_t*> out = as_const(a.out_tab) + static_cast<size_t>(stripe) * R;
  const bool active = v0 < nvec;
  auto ld = [&](int i) {
    Src s;
    if constexpr (PAIR) {
      s.a = load16<P>(reinterpret_cast<const uint4*>(in[2 * i]) + v0);
      s.b = load16<P>(reinterpret_cast<const uint4*>(in[2 * i + 1]) + v0);
    } else {
      s.a = load16<P>(reinterpret_cast<const uint4*>(in[i]) + v0);
    }
    return s;
  };
  // The first sources go out before the table prologue, as in mixed_tile.
  Src xr[NR];
#pragma unroll
  for (int s = 0; s < NR; ++s) {
    xr[s].a = make_uint4(0, 0, 0, 0);
    if constexpr (PAIR) xr[s].b = make_uint4(0, 0, 0, 0);
  }
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
    if (j != ~0u) update_tail<RT, PAIR>(S, nvec, C, R, in, out, lds0, j);
  }
  if (!active) return;
  AccT acc[4][4];
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[w][j] = lds_zero<RT>();
  constexpr bool kVpf = P::VPF > 0;
  static_assert(!kVpf || RT <= 4, "early destination loads: RT <= 4 only");
  uint4 vpre[kVpf ? RT : 1];
#pragma unroll
  for (int r = 0; r < (kVpf ? RT : 1); ++r) vpre[r] = make_uint4(0, 0, 0, 0);
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
        lds_mac<RT, P::SDWA>(acc, update_delta<PAIR>(xr[s]), lds0 + static_cast<uint32_t>(i) * 32u * W);
      }
    }
  }

  // every row: the destination's 16 bytes XOR the row, stored where they were loaded
  if constexpr (kVpf) {
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
