// Owners of raw memory: a device block (hipMalloc / hipFree) and a pinned host block (hipHostMalloc / hipHostFree).
// Move-only; the destructor releases.  Nothing here knows pdeopt_ctx: the callers turn a hipError_t into their own error
// (ensure_buffer / grow_device_buffer of common.hpp).  The HIP device in effect is the caller's business.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace pdeopt {

// device bytes currently held through DeviceBuffer, process-wide (PDEOPT_CNT_DEVICE_BYTES)
inline std::atomic<int64_t> g_device_bytes{0};

namespace detail {
struct DeviceMem {
  static hipError_t alloc(void** p, size_t n) {
    const hipError_t e = hipMalloc(p, n);
    if (e == hipSuccess) g_device_bytes += (int64_t)n;
    return e;
  }
  static void release(void* p, size_t n) {
    (void)hipFree(p);
    g_device_bytes -= (int64_t)n;
  }
};
struct PinnedMem {
  static hipError_t alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
  static void release(void* p, size_t) { (void)hipHostFree(p); }
};

template <typename Mem>
class Buffer {
 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { reset(); }

  void* get() const { return p_; }
  template <typename T>
  T* as() const { return static_cast<T*>(p_); }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() {
    if (p_) Mem::release(p_, bytes_);
    p_ = nullptr;
    bytes_ = 0;
  }
  // Allocate when empty.  A block that exists must already hold `bytes`: hipErrorInvalidValue otherwise, and the
  // block stays as it is.  A failed allocation leaves the buffer empty.
  hipError_t ensure(size_t bytes) {
    if (p_) return bytes_ >= bytes ? hipSuccess : hipErrorInvalidValue;
    const hipError_t e = Mem::alloc(&p_, bytes);
    if (e != hipSuccess) p_ = nullptr;
    else bytes_ = bytes;
    return e;
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};
}  // namespace detail

using PinnedBuffer = detail::Buffer<detail::PinnedMem>;

class DeviceBuffer : public detail::Buffer<detail::DeviceMem> {
 public:
  // Grow-only: a block that is too small is freed and a new one allocated; never shrinks.
  hipError_t reserve(size_t bytes) {
    if (*this && this->bytes() < bytes) reset();
    return ensure(bytes);
  }
};

}  // namespace pdeopt
