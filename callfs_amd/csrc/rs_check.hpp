// Final decode-check launches: progressive Verify on the device. The block
// body of rs_merge_ragged (rs_merge.hpp: the ragged block setup, the first source loads ahead of
// the table prologue, the same ring, lds_mac, non-temporal accesses and plain unaligned 16-byte
// accesses, the pattern's own row count) plus a block-uniform cmask, read beside nrows[p]: bit r
// marks row r as a check row. A check row is never stored. The value it would have received --
// the computed row XORed into the accumulator's bytes, or under STORE the computed row alone,
// with nothing of the accumulator read -- is ORed into a per-lane flag, in the vector path and
// in the S % 16 tail alike, and a wave that saw a nonzero byte ORs 1 into the stripe's status
// word with one atomic. Wanted rows are merged or stored as in rs_merge_ragged. A pattern with no
// source (nsrc[p] == 0) loads no source and copies no table: its accumulators are only scanned.
// Included by rs_mixed.hip alone.
#pragma once

#include "rs_merge.hpp"

namespace callfs {
namespace dev {

// merge_tail with check rows: returns whether a check row's value at byte 16 * nvec + j is
// nonzero.
template <int RT, bool STORE>
__device__ __forceinline__ bool check_tail(uint64_t S, uint64_t nvec, int C, int R, uint32_t cmask,
                                           cptr<const uint8_t*> in, cptr<uint8_t*> out,
                                           uint32_t lds0, uint32_t j) {
  constexpr int W = LdsAcc<RT>::W;
  const uint32_t nt = static_cast<uint32_t>(S - nvec * 16);
  if (j >= nt) return false;
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
  uint32_t bad = 0;
  for (int r = 0; r < R && r < RT; ++r) {
    uint32_t v = lds_byte<RT>(t, r) & 0xffu;
    if constexpr (!STORE) v ^= out[r][b];
    if ((cmask >> r) & 1u) bad |= v;
    else out[r][b] = static_cast<uint8_t>(v);
  }
  return bad != 0;
}

// Instances, tiles and the tile map as for rs_merge_ragged.
template <int RT, class P, bool STORE>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_check_ragged(ApplyArgs a, CheckArgs xc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int BS = P::BS;
  constexpr int W = LdsAcc<RT>::W;
  constexpr int PD = P::PD, NR = P::PD + 1;
  static_assert(P::TILE_VECS == BS, "one vector per thread: the tile map counts 512-vector tiles");
  using AccT = typename LdsAcc<RT>::T;
  const UpdateArgs& x = xc.m.u;
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  // the stripe, its tile, its size, its pattern and the pattern's source count, row count and
  // check rows: all wave-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  const uint64_t S = as_const(x.size)[stripe];
  const uint64_t nvec = S / 16;
  const int C = static_cast<int>(as_const(x.nsrc)[p]);
  const int R = static_cast<int>(as_const(xc.m.nrows)[p]);
  const uint32_t cmask = as_const(xc.cmask)[p];
  if (R == 0) return;  // block-uniform
  const uint64_t v0 = static_cast<uint64_t>(tile) * BS + threadIdx.x;
  cptr<const uint8_t*> in = as_const(a.in_tab) + static_cast<size_t>(stripe) * x.in_stride;
  cptr<uint8_t*> out = as_const(a.out_tab) + static_cast<size_t>(stripe) * a.R;
  const bool active = v0 < nvec;
  auto ld = [&](int i) { return load16<P>(reinterpret_cast<const uint4*>(in[i]) + v0); };
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
  bool bad = false;
  if (a.tail_in_vec) {
    const uint32_t j = tail_lane<BS>(a.tail_in_vec, tile);
    if (j != ~0u) bad = check_tail<RT, STORE>(S, nvec, C, R, cmask, in, out, lds0, j);
  }
  if (active) {
    AccT acc[4][4];
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[w][j] = lds_zero<RT>();
    // the early accumulator and destination loads of RT 4, as in rs_merge_ragged
    constexpr bool kVpf = P::VPF > 0 && !STORE;
    static_assert(!kVpf || RT <= 4, "early destination loads: RT <= 4 only");
    uint4 vpre[kVpf ? RT : 1];
    if constexpr (kVpf) {
#pragma unroll
      for (int r = 0; r < RT; ++r) vpre[r] = make_uint4(0, 0, 0, 0);
    }
    const int vat = C > P::VPF ? C - P::VPF : 0;
    auto pre = [&]() {
      if constexpr (kVpf) {
#pragma unroll
        for (int r = 0; r < RT; ++r)
          if (r < R) vpre[r] = load16<P>(reinterpret_cast<const uint4*>(out[r]) + v0);
      }
    };
    if (C == 0) pre();  // wave-uniform: no source step to issue them from

#pragma unroll 1
    for (int i0 = 0; i0 < C; i0 += NR) {
#pragma unroll
      for (int s = 0; s < NR; ++s) {
        const int i = i0 + s;
        if (i < C) {
          if (i + PD < C) xr[(s + PD) % NR] = ld(i + PD);
          if (i == vat) pre();
          lds_mac<RT, P::SDWA>(acc, xr[s], lds0 + static_cast<uint32_t>(i) * 32u * W);
        }
      }
    }

    auto row = [&](int r) {
      return make_uint4(lds_row<RT>(acc[0], r), lds_row<RT>(acc[1], r), lds_row<RT>(acc[2], r),
                        lds_row<RT>(acc[3], r));
    };
    // row r's value v: tested if r is a check row (wave-uniform), stored if not
    auto put = [&](int r, const uint4& v) {
      if ((cmask >> r) & 1u) bad |= (v.x | v.y | v.z | v.w) != 0;
      else store16<P>(reinterpret_cast<uint4*>(out[r]) + v0, v);
    };
    if constexpr (STORE) {
      // every row as computed: nothing of a destination or an accumulator is read
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r >= R) continue;  // wave-uniform
        put(r, row(r));
      }
    } else if constexpr (kVpf) {
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r >= R) continue;  // wave-uniform
        const uint4 y = vpre[r], o = row(r);
        put(r, make_uint4(y.x ^ o.x, y.y ^ o.y, y.z ^ o.z, y.w ^ o.w));
      }
    } else {
      // four rows' loads in flight, then their four stores or tests
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
          const uint4 o = row(r);
          put(r, make_uint4(y[q].x ^ o.x, y[q].y ^ o.y, y[q].z ^ o.z, y[q].w ^ o.w));
        }
      }
    }
  }
  // one atomic per wave that saw a nonzero value, by its first such lane
  const uint64_t saw = __ballot(bad);
  if (bad && (threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(saw)))
    atomicOr(a.status + static_cast<size_t>(stripe) * a.status_stride, 1);
}

}  // namespace dev
}  // namespace callfs
