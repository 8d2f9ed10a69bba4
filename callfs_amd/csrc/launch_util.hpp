// Launch helpers shared by the kernel files (rs_kernels.hip, rs_mixed.hip): one dispatch
// with optional start / stop events, and a long grid cut into equal consecutive slices.
// HIP only; internal to the library.
#pragma once

#include <algorithm>
#include <cstdint>

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "rs_kernels.hpp"

namespace callfs {

// One dispatch of kernel fn; with events, the first dispatch of a launch records ev.start
// at its start and the last records ev.stop at its end (hipExtLaunchKernel).
template <class... Args>
void dispatch(void (*fn)(Args...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
              const LaunchEvents& ev, bool first, bool last, Args... args) {
  if (ev.start || ev.stop)
    hipExtLaunchKernelGGL(fn, grid, block, static_cast<uint32_t>(lds), stream,
                          first ? ev.start : nullptr, last ? ev.stop : nullptr, 0, args...);
  else
    hipLaunchKernelGGL(fn, grid, block, lds, stream, args...);
}

// Cuts `grid` blocks into equal consecutive slices of at most `lim` blocks (one slice when
// the grid is no more than twice `lim`) and calls launch(blocks, first, last) for each with
// a.t_base set to the slice's first block; first / last = the grid's first / last slice.
template <class Launch>
void launch_slices(uint32_t grid, uint32_t lim, ApplyArgs& a, Launch&& launch) {
  const uint32_t nsl = grid / 2 > lim ? (grid + lim - 1) / lim : 1;
  const uint32_t per = (grid + nsl - 1) / nsl;
  for (uint32_t t0 = 0; t0 < grid; t0 += per) {
    a.t_base = t0;
    launch(std::min(per, grid - t0), t0 == 0, t0 + per >= grid);
  }
  a.t_base = 0;
}

}  // namespace callfs
