// lol_amd/csrc/devmem.h — who frees device memory, stated once: every allocation belongs to a DevBuf
// (hipMalloc, freed with its owner) or a StreamBuf (stream-ordered, freed on the caller's stream), so a handle's destroy
// entry is `delete` and a create that fails frees what was live by returning.  Host code only.  No owner has static
// storage duration: a destructor that ran after the HIP runtime's shutdown would call into it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

#include "lolhip.h"

namespace lolhip {

// one hipMalloc allocation of T: empty by default, move-only, as large as the pointer it replaces
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
  int alloc(size_t count) {
    reset();
    if (hipMalloc((void**)&p_, count * sizeof(T)) == hipSuccess) return LOLHIP_OK;
    p_ = nullptr;
    return LOLHIP_ERR_HIP;
  }
  // a synchronous copy of h; an empty h leaves the buffer null
  int upload(const std::vector<T>& h) {
    reset();
    if (h.empty()) return LOLHIP_OK;
    if (int rc = alloc(h.size())) return rc;
    return hipMemcpy(p_, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};

// stream-ordered workspace: allocated and released on the caller's stream, so concurrent calls on
// one plan (other host threads, other streams) never share it and nothing synchronises the device
struct StreamBuf {
  void* p = nullptr;
  hipStream_t s;
  explicit StreamBuf(hipStream_t s_) : s(s_) {}
  ~StreamBuf() { if (p) (void)hipFreeAsync(p, s); }
  bool alloc(size_t bytes) { return hipMallocAsync(&p, bytes ? bytes : 8, s) == hipSuccess; }
};

// a private non-blocking stream for the work of a create.  Declare it AFTER the buffers its work touches: the destructor
// drains the stream, on error paths too, before those buffers are freed.
class ScopedStream {
 public:
  ScopedStream() { if (hipStreamCreateWithFlags(&s_, hipStreamNonBlocking) != hipSuccess) s_ = nullptr; }
  ~ScopedStream() { if (s_) { (void)hipStreamSynchronize(s_); (void)hipStreamDestroy(s_); } }
  ScopedStream(const ScopedStream&) = delete;
  ScopedStream& operator=(const ScopedStream&) = delete;
  bool ok() const { return s_ != nullptr; }
  int sync() { return hipStreamSynchronize(s_) == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP; }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace lolhip
