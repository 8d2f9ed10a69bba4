// The rest of the HIP runtime that the device-plan code (rs_plan.cpp, rs_context.cpp) calls,
// beside the launch entry points of fake_hip_runtime.cpp: one device, "device" memory that is
// host memory, streams and events that do nothing. Every host-to-device hipMemcpy is kept in
// fake_mem::uploads, so a program can read what a plan put into its device buffer.
#include "fake_hip_memory.hpp"

#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>

#include "bitslice.hpp"

namespace fake_mem {
std::vector<std::vector<unsigned char>>& uploads() {
  static std::vector<std::vector<unsigned char>> u;
  return u;
}
AsyncCopies& async_copies() {
  static AsyncCopies c;
  return c;
}
}  // namespace fake_mem

extern "C" {
hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) {
  *p = std::malloc(n ? n : 1);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
  std::free(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return hipMalloc(p, n); }
hipError_t hipHostFree(void* p) { return hipFree(p); }
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
  std::memcpy(dst, src, n);
  if (kind == hipMemcpyHostToDevice) {
    const auto* b = static_cast<const unsigned char*>(src);
    fake_mem::uploads().emplace_back(b, b + n);
  }
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t) {
  std::memcpy(dst, src, n);
  if (kind == hipMemcpyHostToDevice) ++fake_mem::async_copies().h2d;
  if (kind == hipMemcpyDeviceToHost) ++fake_mem::async_copies().d2h;
  return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t n) {
  std::memset(dst, v, n);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int v, size_t n, hipStream_t) {
  std::memset(dst, v, n);
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  *s = nullptr;
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) {
  *st = hipStreamCaptureStatusNone;
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = nullptr;
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  *e = nullptr;
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  *ms = 1.0f;
  return hipSuccess;
}
}  // extern "C"

namespace callfs {
namespace bs {
std::shared_ptr<Kernel> kernel_for(int K, int R, const uint8_t* coef) {
  return std::make_shared<Kernel>(K, R, coef);
}
}  // namespace bs
}  // namespace callfs
