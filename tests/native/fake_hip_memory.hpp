// Stand-ins for the memory, stream and event calls of the HIP runtime (fake_hip_memory.cpp),
// for programs that run the device-plan code on a machine without a GPU beside the
// recording launch entry points of fake_hip_runtime.hpp.
#pragma once

#include <vector>

namespace fake_mem {

// The bytes of every host-to-device hipMemcpy, in order.
std::vector<std::vector<unsigned char>>& uploads();

// How many hipMemcpyAsync calls went each way.
struct AsyncCopies {
  long h2d = 0, d2h = 0;
};
AsyncCopies& async_copies();

}  // namespace fake_mem
