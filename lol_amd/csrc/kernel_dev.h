// lol_amd/csrc/kernel_dev.h — per-device launch state of one kernel instantiation (host code only).
// hipFuncSetAttribute is per DEVICE: a process that drives several GPUs has to repeat it on each of them (a
// per-process flag made the second GPU's first > 64 KiB-LDS launch fail).  state 0 = not set up, 2 = ready.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <mutex>

namespace lolhip {

constexpr int MAX_DEV = 64;
struct KernelDev { std::atomic<int> state{0}; };
inline std::mutex& kernel_dev_mutex() { static std::mutex m; return m; }
template <typename Setup>
static hipError_t kernel_dev_setup(KernelDev (&tab)[MAX_DEV], Setup&& setup) {
  int dev = -1;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= MAX_DEV) return hipErrorInvalidDevice;
  KernelDev& d = tab[dev];
  if (d.state.load(std::memory_order_acquire) != 2) {
    std::lock_guard<std::mutex> g(kernel_dev_mutex());
    if (d.state.load(std::memory_order_relaxed) != 2) {
      e = setup();
      if (e != hipSuccess) return e;
      d.state.store(2, std::memory_order_release);
    }
  }
  return hipSuccess;
}

// the usual setup: kernel K may take `bytes` of dynamic LDS (more than the 64 KiB a kernel gets unasked)
template <auto K>
static hipError_t allow_big_lds(int bytes) {
  static KernelDev tab[MAX_DEV];
  return kernel_dev_setup(tab, [&]() -> hipError_t {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  });
}

}  // namespace lolhip
