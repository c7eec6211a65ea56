// Stand-alone check of csrc/device_buffer.hpp against counting stubs of the HIP allocation calls.  Built host-only with
// -fsanitize=address,undefined and run as a child process by tests/test_device_buffer_cpu.py: a double free, a leak or a
// use after free ends the program with a sanitizer report, a wrong count with a line number and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "device_buffer.hpp"

static int n_malloc = 0, n_free = 0, n_host_malloc = 0, n_host_free = 0;
static bool fail_next = false;

hipError_t hipMalloc(void** p, size_t n) {
  if (fail_next) {
    fail_next = false;
    *p = reinterpret_cast<void*>(0x1);  // what a failed call leaves behind is not to be trusted
    return hipErrorOutOfMemory;
  }
  ++n_malloc;
  *p = std::malloc(n ? n : 1);
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  ++n_free;
  std::free(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned) {
  if (fail_next) {
    fail_next = false;
    *p = reinterpret_cast<void*>(0x1);
    return hipErrorOutOfMemory;
  }
  ++n_host_malloc;
  *p = std::malloc(n ? n : 1);
  return hipSuccess;
}
hipError_t hipHostFree(void* p) {
  ++n_host_free;
  std::free(p);
  return hipSuccess;
}

#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);     \
      return 1;                                                 \
    }                                                           \
  } while (0)

using pdeopt::DeviceBuffer;
using pdeopt::PinnedBuffer;
using pdeopt::g_device_bytes;

static int run() {
  {  // the destructor frees once
    DeviceBuffer b;
    CHECK(!b && b.get() == nullptr && b.bytes() == 0);
    CHECK(b.ensure(100) == hipSuccess);
    CHECK(b && b.bytes() == 100 && n_malloc == 1 && g_device_bytes == 100);
    b.as<char>()[99] = 1;
  }
  CHECK(n_free == 1 && g_device_bytes == 0);
  {  // reset is idempotent
    DeviceBuffer b;
    CHECK(b.ensure(8) == hipSuccess);
    b.reset();
    b.reset();
    CHECK(!b && b.bytes() == 0 && n_free == 2);
  }
  CHECK(n_free == 2);
  {  // move construction and assignment leave the source empty; std::swap exchanges owners
    DeviceBuffer a, b;
    CHECK(a.ensure(16) == hipSuccess && b.ensure(32) == hipSuccess);
    void *pa = a.get(), *pb = b.get();
    std::swap(a, b);
    CHECK(a.get() == pb && a.bytes() == 32 && b.get() == pa && b.bytes() == 16 && n_free == 2);
    DeviceBuffer c(std::move(a));
    CHECK(!a && a.bytes() == 0 && c.get() == pb && c.bytes() == 32);
    b = std::move(c);  // frees the 16-byte block
    CHECK(!c && b.get() == pb && n_free == 3 && g_device_bytes == 32);
    DeviceBuffer& self = b;
    b = std::move(self);
    CHECK(b.get() == pb && n_free == 3);
  }
  CHECK(n_malloc == 4 && n_free == 4 && g_device_bytes == 0);
  {  // ensure: empty, large enough, too small
    DeviceBuffer b;
    CHECK(b.ensure(64) == hipSuccess);
    void* p = b.get();
    CHECK(b.ensure(64) == hipSuccess && b.ensure(10) == hipSuccess && b.get() == p && b.bytes() == 64 && n_malloc == 5);
    CHECK(b.ensure(65) == hipErrorInvalidValue && b.get() == p && b.bytes() == 64 && n_malloc == 5 && n_free == 4);
    // reserve: never shrinks, frees the old block exactly once when it grows
    CHECK(b.reserve(32) == hipSuccess && b.get() == p && b.bytes() == 64 && n_malloc == 5 && n_free == 4);
    CHECK(b.reserve(128) == hipSuccess && b.bytes() == 128 && n_malloc == 6 && n_free == 5 && g_device_bytes == 128);
    b.as<char>()[127] = 1;
    // a failed allocation leaves the buffer empty
    fail_next = true;
    CHECK(b.reserve(256) == hipErrorOutOfMemory && !b && b.get() == nullptr && b.bytes() == 0 && n_free == 6 && g_device_bytes == 0);
    fail_next = true;
    CHECK(b.ensure(8) == hipErrorOutOfMemory && !b && b.bytes() == 0);
    CHECK(b.ensure(8) == hipSuccess && b.bytes() == 8);
  }
  CHECK(n_malloc == 7 && n_free == 7 && g_device_bytes == 0);
  {  // the pinned sibling
    PinnedBuffer a, b;
    CHECK(a.ensure(24) == hipSuccess && a.ensure(25) == hipErrorInvalidValue && a.bytes() == 24);
    b = std::move(a);
    CHECK(!a && b.bytes() == 24 && n_host_malloc == 1 && n_host_free == 0);
    fail_next = true;
    CHECK(a.ensure(8) == hipErrorOutOfMemory && !a);
    CHECK(g_device_bytes == 0);  // pinned memory is not device memory
  }
  CHECK(n_host_malloc == 1 && n_host_free == 1);
  CHECK(n_malloc == n_free && g_device_bytes == 0);
  return 0;
}

int main() {
  const int rc = run();
  if (rc == 0) std::printf("device_buffer ok: %d device and %d pinned blocks, all freed\n", n_malloc, n_host_malloc);
  return rc;
}
