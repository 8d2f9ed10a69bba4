// The recording stand-in described in fake_hip_runtime.hpp: the handful of HIP entry points a
// host-only build of rs_kernels.hip calls, and the five bit-sliced runtime functions it uses.
#include "fake_hip_runtime.hpp"

#include <cstdarg>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "bitslice.hpp"
#include "rs_kernels.hpp"

namespace fake {
std::string log;
bool recording = true;
int device = 40;
int bs_ready = 0;
int bs_mode = 1;

std::map<std::string, long>& kernels() {
  static std::map<std::string, long> m;
  return m;
}

namespace {
std::map<const void*, std::string>& stubs() {
  static std::map<const void*, std::string> m;
  return m;
}
struct CallConfig {
  dim3 grid, block;
  size_t lds = 0;
  hipStream_t stream = nullptr;
} g_cfg;

void linef(const char* f, ...) __attribute__((format(printf, 1, 2)));
void linef(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  log += buf;
}

hipError_t record(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, const char* ev) {
  if (!recording) return hipSuccess;
  auto it = stubs().find(fn);
  const std::string name = it == stubs().end() ? "?" : it->second;
  if (it != stubs().end()) ++kernels()[name];
  linef("  %s grid=%u,%u block=%u lds=%zu", name.c_str(), grid.x, grid.y, block.x, lds);
  if (name.find("rs_apply_small") == std::string::npos) {
    const auto* a = static_cast<const callfs::ApplyArgs*>(args[0]);
    linef(" nvec=%llu t_base=%u tiv=%u", static_cast<unsigned long long>(a->nvec), a->t_base,
          a->tail_in_vec);
    if (name.find("rs_apply_bytes") != std::string::npos)
      linef(" tail0=%llu", static_cast<unsigned long long>(*static_cast<const uint64_t*>(args[1])));
  }
  linef(" ev=%s\n", ev);
  return hipSuccess;
}
const char* ev_name(hipEvent_t start, hipEvent_t stop) {
  return start ? (stop ? "start+stop" : "start") : (stop ? "stop" : "-");
}
}  // namespace
}  // namespace fake

extern "C" {
void** __hipRegisterFatBinary(const void*) {
  static void* handle = nullptr;
  return &handle;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned,
                           void*, void*, void*, void*, int*) {
  fake::stubs()[host_fn] = device_name;
  fake::kernels()[device_name];
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
  fake::g_cfg = {grid, block, lds, stream};
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
  *grid = fake::g_cfg.grid;
  *block = fake::g_cfg.block;
  *lds = fake::g_cfg.lds;
  *stream = fake::g_cfg.stream;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds,
                           hipStream_t) {
  return fake::record(fn, grid, block, args, lds, "none");
}
hipError_t hipExtLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds,
                              hipStream_t, hipEvent_t start, hipEvent_t stop, int) {
  return fake::record(fn, grid, block, args, lds, fake::ev_name(start, stop));
}
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipGetDevice(int* d) {
  *d = fake::device;
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute attr, int value) {
  if (!fake::recording) return hipSuccess;
  auto it = fake::stubs().find(fn);
  fake::linef("  attr %s %d=%d\n", it == fake::stubs().end() ? "?" : it->second.c_str(),
              static_cast<int>(attr), value);
  return hipSuccess;
}
}  // extern "C"

namespace callfs {
namespace bs {
Kernel::Kernel(int K, int R, const uint8_t*) {
  net_.K = K;
  net_.R = R;
}
Kernel::~Kernel() = default;
Kernel::State Kernel::state() const { return fake::bs_ready ? State::kReady : State::kIdle; }
void Kernel::compile_async() {
  if (fake::recording) fake::linef("  bs compile_async\n");
}
hipFunction_t Kernel::function(int, bool wait) {
  if (!fake::bs_ready && fake::recording) fake::linef("  bs function wait=%d\n", wait ? 1 : 0);
  return fake::bs_ready || wait ? reinterpret_cast<hipFunction_t>(this) : nullptr;
}
Mode mode() { return static_cast<Mode>(fake::bs_mode); }
hipError_t launch(hipFunction_t, const Args& a, uint32_t tiles, int block, hipStream_t,
                  hipEvent_t start, hipEvent_t stop) {
  if (fake::recording)
    fake::linef("  rs_bs tiles=%u block=%d nvec=%llu tps=%u ntiles=%u t_base=%u vm=%#x order=%d ev=%s\n",
                tiles, block, static_cast<unsigned long long>(a.nvec), a.tps, a.ntiles, a.t_base,
                a.verify_mask, a.order, fake::ev_name(start, stop));
  return hipSuccess;
}
}  // namespace bs
}  // namespace callfs
