// A stand-in for the HIP runtime and the bit-sliced kernel runtime (bitslice.cpp) that records
// what rs_kernels.hip launches instead of launching it (fake_hip_runtime.cpp). It lets
// launch_record.cpp observe kernel selection, grids, LDS sizes, tail placement and slicing on a
// machine without a GPU: the kernel file is compiled for the host only and linked against
// this, with none of the real runtime.
#pragma once

#include <cstdint>
#include <map>
#include <string>

namespace fake {

// Every dispatch, attribute call and bit-sliced compile request appends one line here while
// `recording` is set.
extern std::string log;
extern bool recording;

// hipGetDevice's answer. Devices outside [0, 32) make dispatch.hpp's DeviceOnce run its
// function every time, so a case's record does not depend on the cases before it.
extern int device;

// What the fake bs::Kernel and bs::mode() report: 0 = not compiled, 1 = ready; bs_mode as
// bs::Mode's values (0 off, 1 auto, 2 sync).
extern int bs_ready;
extern int bs_mode;

// Registered kernels (device symbol -> number of dispatches recorded).
std::map<std::string, long>& kernels();

}  // namespace fake
