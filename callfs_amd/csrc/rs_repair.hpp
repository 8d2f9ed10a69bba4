// Decode-repair launches: the final launch of a progressive decode that names
// the corrupt shard of a mismatching byte column from the finished check rows, repairs the wanted
// rows within the launch and hands the error values back. The clean path is rs_check_ragged's
// body (rs_check.hpp: the ragged block setup, the first source loads ahead of the table prologue,
// the same ring and lds_mac, the early accumulator loads at RT 4, the nsrc[p] == 0 scan) with the
// rows ordered check rows first: every check row is tested before any wanted row is stored, and
// one ballot after them decides. Every wave then stores its wanted rows as rs_check_ragged does,
// and a wave with no mismatching lane leaves. The slow path follows rs_apply_correct's pattern
// (rs_mixed.hip mixed_tile LOCATE 3, §5.13): in merge mode the check rows' old bytes are XORed
// into the transposed accumulators, so that acc[w][j] holds the syndromes of column 4 w + j; a
// mismatching lane classifies its 16 columns with locate_correct (the tables are read from
// global memory, the path is rare) in one loop that is not unrolled, the column picked out of the
// accumulators with selects, so that the kernel holds one copy of the rule and the accumulators
// stay in registers; the error values of the shard the current run blames are gathered into one
// 16-byte vector, and when the verdict changes and at the end that vector is XORed into the
// shard's fix buffer (a lane-variant load of the pointer; null: count only) and, for an expected
// shard at position j, G[r][j] times it into the 16 bytes of every wanted row r the lane has
// just stored (repair_mul_word: the accumulators are only read, and the lane reads back what it
// wrote itself). Written into the accumulators before one store instead, the repair took 37
// registers more at 16 rows. Counts go through locate_wave_add, the status word takes one
// atomic per wave, and nothing block-wide follows the prologue's barrier.
// Included by rs_mixed.hip alone, behind its locate helpers (lds_xor_byte, locate_words,
// locate_wave_add).
#pragma once

#include "decode_repair_tables.hpp"
#include "rs_check.hpp"

namespace callfs {
namespace dev {

// lds_xor_byte for a row that is not static: selects, not an indexed word (a runtime index into
// t.v would put the accumulators in scratch).
template <int RT>
__device__ __forceinline__ void repair_xor_byte(typename LdsAcc<RT>::T& t, int r, uint32_t b) {
  if constexpr (RT > 8) {
    const uint32_t add = b << (8 * (r & 3));
#pragma unroll
    for (int d = 0; d < 4; ++d) t.v[d] ^= (r >> 2) == d ? add : 0u;
  } else if constexpr (RT > 4) {
    t ^= static_cast<uint64_t>(b) << (8 * r);
  } else {
    t ^= b << (8 * r);
  }
}

// The S % 16 tail of a decode-repair launch: check_tail with the byte's column classified and
// repaired, one byte per thread. Every thread of the waves that call it reaches the ballots.
template <int RT, bool STORE>
__device__ __forceinline__ void repair_tail(const ApplyArgs& a, const RepairArgs& xr, uint64_t S, uint64_t nvec,
                                            int C, int R, int nchk, cptr<const uint8_t*> in, cptr<uint8_t*> out,
                                            uint32_t stripe, uint32_t p, uint32_t lds0, uint32_t j) {
  constexpr int W = LdsAcc<RT>::W;
  const uint32_t nt = static_cast<uint32_t>(S - nvec * 16);
  uint32_t v = kLocateClean;
  if (j < nt) {
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
    if constexpr (!STORE) {
#pragma unroll
      for (int r = 0; r < RT; ++r)
        if (r < R) lds_xor_byte<RT>(t, r, out[r][b]);
    }
    uint32_t s[RT / 4];
    locate_words<RT>(t, s);
    uint32_t pos = 0, val = 0;
    v = repair_column(s, nchk, R, xr.k, xr.gf, xr.loc + static_cast<size_t>(p) * xr.loc_stride, pos, val);
    if (v < 256u) {
      uint8_t* f = xr.fix[static_cast<size_t>(stripe) * fix_slots(xr.k) + pos];
      if (f) f[b] ^= static_cast<uint8_t>(val);
    }
#pragma unroll
    for (int r = 0; r < RT; ++r)
      if (r >= nchk && r < R) out[r][b] = static_cast<uint8_t>(locate_byte(s, r));
  }
  const uint64_t saw = __ballot(v != kLocateClean);
  if (saw == 0) return;  // wave-uniform
  if ((threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(saw)))
    atomicOr(a.status + static_cast<size_t>(stripe) * a.status_stride, 1);
  locate_wave_add<false>(xr.counts + static_cast<size_t>(stripe) * xr.nbins, xr.nbins, v, v != kLocateClean ? 1u : 0u);
}

// Instances, tiles and the tile map as for rs_check_ragged.
template <int RT, class P, bool STORE>
__global__ __launch_bounds__(P::BS) __attribute__((amdgpu_waves_per_eu(P::WPE, lds_max_waves<RT>())))
void rs_repair_ragged(ApplyArgs a, RepairArgs xr) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int BS = P::BS;
  constexpr int W = LdsAcc<RT>::W;
  constexpr int PD = P::PD, NR = P::PD + 1;
  static_assert(P::TILE_VECS == BS, "one vector per thread: the tile map counts 512-vector tiles");
  using AccT = typename LdsAcc<RT>::T;
  const UpdateArgs& x = xr.c.m.u;
  const uint32_t t = a.t_base + blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  // the stripe, its tile, its size, its pattern and the pattern's source count, row count and
  // check rows (rows [0, nchk): cmask is the low nchk bits): all wave-uniform
  const uint32_t stripe = as_const(x.tile_stripe)[t];
  const uint32_t tile = t - as_const(x.tile0)[stripe];
  const uint32_t p = as_const(x.pat)[stripe];
  const uint64_t S = as_const(x.size)[stripe];
  const uint64_t nvec = S / 16;
  const int C = static_cast<int>(as_const(x.nsrc)[p]);
  const int R = static_cast<int>(as_const(xr.c.m.nrows)[p]);
  const int nchk = __builtin_popcount(as_const(xr.c.cmask)[p]);
  if (R == 0) return;  // block-uniform
  const uint64_t v0 = static_cast<uint64_t>(tile) * BS + threadIdx.x;
  cptr<const uint8_t*> in = as_const(a.in_tab) + static_cast<size_t>(stripe) * x.in_stride;
  cptr<uint8_t*> out = as_const(a.out_tab) + static_cast<size_t>(stripe) * a.R;
  const bool active = v0 < nvec;
  auto ld = [&](int i) { return load16<P>(reinterpret_cast<const uint4*>(in[i]) + v0); };
  uint4 xs[NR];
#pragma unroll
  for (int s = 0; s < NR; ++s) xs[s] = make_uint4(0, 0, 0, 0);
  if (active) {
#pragma unroll
    for (int s = 0; s < PD; ++s)
      if (s < C) xs[s] = ld(s);
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
    if (j != ~0u) repair_tail<RT, STORE>(a, xr, S, nvec, C, R, nchk, in, out, stripe, p, lds0, j);
  }
  if (!active) return;
  AccT acc[4][4];
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[w][j] = lds_zero<RT>();
  // the early accumulator and destination loads of RT 4, as in rs_check_ragged
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
        if (i + PD < C) xs[(s + PD) % NR] = ld(i + PD);
        if (i == vat) pre();
        lds_mac<RT, P::SDWA>(acc, xs[s], lds0 + static_cast<uint32_t>(i) * 32u * W);
      }
    }
  }

  auto row = [&](int r) {
    return make_uint4(lds_row<RT>(acc[0], r), lds_row<RT>(acc[1], r), lds_row<RT>(acc[2], r),
                      lds_row<RT>(acc[3], r));
  };
  auto old = [&](int r) { return load16<P>(reinterpret_cast<const uint4*>(out[r]) + v0); };
  // rows [lo, hi) (wave-uniform bounds): row r's value handed to f; in merge mode without the
  // early loads four rows' loads are in flight before the first is used
  auto rows = [&](int lo, int hi, auto f) {
    if constexpr (STORE) {
#pragma unroll
      for (int r = 0; r < RT; ++r)
        if (r >= lo && r < hi) f(r, row(r));
    } else if constexpr (kVpf) {
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r < lo || r >= hi) continue;
        const uint4 y = vpre[r], o = row(r);
        f(r, make_uint4(y.x ^ o.x, y.y ^ o.y, y.z ^ o.z, y.w ^ o.w));
      }
    } else {
#pragma unroll
      for (int r0 = 0; r0 < RT; r0 += 4) {
        if (r0 + 4 <= lo || r0 >= hi) continue;  // wave-uniform
        uint4 y[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          y[q] = make_uint4(0, 0, 0, 0);
          if (r0 + q >= lo && r0 + q < hi) y[q] = old(r0 + q);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = r0 + q;
          if (r < lo || r >= hi) continue;
          const uint4 o = row(r);
          f(r, make_uint4(y[q].x ^ o.x, y[q].y ^ o.y, y[q].z ^ o.z, y[q].w ^ o.w));
        }
      }
    }
  };
  // the check rows first: a wave knows whether it is clean before its first store
  bool bad = false;
  rows(0, nchk, [&](int, const uint4& v) { bad |= (v.x | v.y | v.z | v.w) != 0; });
  const uint64_t saw = __ballot(bad);
  // the wanted rows as rs_check_ragged stores them; a wave with no mismatching lane is done
  rows(nchk, R, [&](int r, const uint4& v) { store16<P>(reinterpret_cast<uint4*>(out[r]) + v0, v); });
  if (saw == 0) return;  // wave-uniform

  // ---- a wave with a mismatching lane: the lanes still here stay together below ----
  if ((threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(saw)))
    atomicOr(a.status + static_cast<size_t>(stripe) * a.status_stride, 1);
  if constexpr (!STORE) {
    // acc's byte r holds check row r's computed byte: XORing the accumulator's in leaves the
    // syndrome
    if constexpr (kVpf) {
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r >= nchk) continue;  // wave-uniform
        const uint32_t yw[4] = {vpre[r].x, vpre[r].y, vpre[r].z, vpre[r].w};
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int j = 0; j < 4; ++j) lds_xor_byte<RT>(acc[w][j], r, (yw[w] >> (8 * j)) & 0xffu);
      }
    } else {
      // one row's load in flight at a time, in a loop that stays a loop: unrolled, the loads of
      // up to 16 rows went out together and took 40 registers more than the clean path holds
#pragma unroll 1
      for (int r = 0; r < nchk; ++r) {
        const uint4 y = old(r);
        const uint32_t yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int j = 0; j < 4; ++j) repair_xor_byte<RT>(acc[w][j], r, (yw[w] >> (8 * j)) & 0xffu);
      }
    }
  }
  const uint8_t* pt = xr.loc + static_cast<size_t>(p) * xr.loc_stride;
  uint64_t* bins = xr.counts + static_cast<size_t>(stripe) * xr.nbins;
  uint8_t* const* fix = xr.fix + static_cast<size_t>(stripe) * fix_slots(xr.k);
  // a lane's columns almost always share one verdict: it keeps (verdict, columns) and the wave
  // adds a lane's run when its verdict changes, and every run at the end (as mixed_tile)
  uint32_t run_v = kLocateClean, run_n = 0;
  auto note = [&](uint32_t v) {
    const bool flush = v != kLocateClean && run_n != 0 && v != run_v;
    if (__ballot(flush) != 0) locate_wave_add<false>(bins, xr.nbins, flush ? run_v : kLocateClean, run_n);
    if (flush) run_n = 0;
    if (v != kLocateClean) {
      run_v = v;
      ++run_n;
    }
  };
  // the error values of the shard the lane's run blames, as the 16 bytes of its own vector. When
  // the verdict changes and at the end they are XORed into the shard's fix buffer with one load
  // and one store, and for an expected shard at position j every wanted row r, stored above,
  // has G[r][j] times them XORed in where it lies. No other lane touches these bytes.
  uint32_t cw[4] = {0, 0, 0, 0}, run_pos = 0;
  auto apply = [&]() {
    uint8_t* f = fix[run_pos];
    if (f) {
      uint4* q = reinterpret_cast<uint4*>(f) + v0;
      uint4 y = load16<P>(q);
      y.x ^= cw[0];
      y.y ^= cw[1];
      y.z ^= cw[2];
      y.w ^= cw[3];
      store16<P>(q, y);
    }
    if (run_pos < static_cast<uint32_t>(xr.k)) {
      const uint8_t* gj = pt + kLocG + static_cast<size_t>(run_pos) * kLocateRows;
#pragma unroll 1
      for (int r = nchk; r < R; ++r) {
        const uint32_t g = gj[r];
        uint4* q = reinterpret_cast<uint4*>(out[r]) + v0;
        uint4 y = load16<P>(q);
        // one word at a time, in a loop that stays a loop: four multiplies side by side held
        // more registers than the clean path has free
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
          const uint32_t o = repair_mul_word(g, i == 0 ? cw[0] : i == 1 ? cw[1] : i == 2 ? cw[2] : cw[3]);
          y.x ^= i == 0 ? o : 0u;
          y.y ^= i == 1 ? o : 0u;
          y.z ^= i == 2 ? o : 0u;
          y.w ^= i == 3 ? o : 0u;
        }
        store16<P>(q, y);
      }
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) cw[w] = 0;
  };
  // one copy of the rule: the column index is wave-uniform and the column's syndromes are picked
  // out of the accumulators with selects, so the accumulators stay in registers (as LOCATE 2)
#pragma unroll 1
  for (int c = 0; c < 16; ++c) {
    uint32_t v = kLocateClean, pos = 0, val = 0;
    if (bad) {
      AccT e = acc[0][0];
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c == w * 4 + j) e = acc[w][j];
      uint32_t s[RT / 4];
      locate_words<RT>(e, s);
      v = locate_correct(s, nchk, xr.k, xr.gf, pt, pos, val);
    }
    if (v != kLocateClean && run_n != 0 && v != run_v && run_v < 256u) apply();
    note(v);
    if (v < 256u) {
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if ((c >> 2) == w) cw[w] |= val << (8 * (c & 3));
      run_pos = pos;
    }
  }
  if (run_n != 0 && run_v < 256u) apply();
  locate_wave_add<false>(bins, xr.nbins, run_n ? run_v : kLocateClean, run_n);
}

}  // namespace dev
}  // namespace callfs
