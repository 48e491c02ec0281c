// Owning handles of the engine's GPU resources: device buffers, page-locked blocks, events, streams.  Each is move-only
// and releases what it holds in its destructor, so a struct built from them (vb_ctx and everything in it) needs no
// release code of its own, and a second owner of one resource does not compile.  This header is the only place in the
// engine that calls the runtime's allocation and creation functions (tests/test_engine_state_cpu.py keeps it so).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

namespace vb {

// resources alive in this process, by kind (vb_resource_counts): the one way to see a release on a device that others share
enum ResourceKind { RES_DEVICE = 0, RES_PINNED, RES_EVENT, RES_STREAM, RES_NUM };
inline std::atomic<uint64_t> g_resources[RES_NUM];
inline void resource_note(int kind, bool born) {
  if (born) g_resources[kind].fetch_add(1, std::memory_order_relaxed);
  else g_resources[kind].fetch_sub(1, std::memory_order_relaxed);
}

struct DeviceBuffer {
  void* ptr = nullptr;      // (public for reading: only alloc / release / moves write them)
  size_t bytes = 0;

  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept { take(o); }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) (void)release(), take(o);
    return *this;
  }
  ~DeviceBuffer() { (void)release(); }

  // plain hipMalloc, no zero fill (vb::ensure adds the fill and the waits); what was held is released first
  hipError_t alloc(size_t n) {
    hipError_t e = release();
    if (e == hipSuccess) e = hipMalloc(&ptr, n);
    if (e != hipSuccess) return ptr = nullptr, e;
    bytes = n;
    resource_note(RES_DEVICE, true);
    return hipSuccess;
  }
  hipError_t release() {
    if (!ptr) return hipSuccess;
    const hipError_t e = hipFree(ptr);
    ptr = nullptr, bytes = 0;
    resource_note(RES_DEVICE, false);
    return e;
  }

 private:
  void take(DeviceBuffer& o) { ptr = o.ptr, bytes = o.bytes, o.ptr = nullptr, o.bytes = 0; }
};

struct PinnedBuffer {
  void* host = nullptr;
  void* dev = nullptr;      // device address of `host` when allocated mapped, else nullptr
  size_t bytes = 0;

  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  PinnedBuffer(PinnedBuffer&& o) noexcept { take(o); }
  PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
    if (this != &o) (void)release(), take(o);
    return *this;
  }
  ~PinnedBuffer() { (void)release(); }

  template <class T> T* host_as() const { return static_cast<T*>(host); }
  template <class T> T* dev_as() const { return static_cast<T*>(dev); }

  hipError_t alloc(size_t n, bool mapped) {
    hipError_t e = release();
    if (e == hipSuccess) e = hipHostMalloc(&host, n, mapped ? hipHostMallocMapped : hipHostMallocDefault);
    if (e != hipSuccess) return host = nullptr, e;
    bytes = n;
    resource_note(RES_PINNED, true);
    return mapped ? hipHostGetDevicePointer(&dev, host, 0) : hipSuccess;
  }
  hipError_t release() {
    if (!host) return hipSuccess;
    const hipError_t e = hipHostFree(host);
    host = dev = nullptr, bytes = 0;
    resource_note(RES_PINNED, false);
    return e;
  }

 private:
  void take(PinnedBuffer& o) { host = o.host, dev = o.dev, bytes = o.bytes, o.host = o.dev = nullptr, o.bytes = 0; }
};

// An event / a stream: converts to the runtime's handle (launches, records and waits read as with a raw handle), tests
// false while empty.  create() is a no-op on a handle that exists: the lazily created ones call it where they are used.
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H), int KIND>
struct Handle {
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) release(), h_ = o.h_, o.h_ = nullptr;
    return *this;
  }
  ~Handle() { release(); }
  operator H() const { return h_; }

  hipError_t create(unsigned flags) {
    if (h_) return hipSuccess;
    const hipError_t e = Create(&h_, flags);
    if (e != hipSuccess) return h_ = nullptr, e;
    resource_note(KIND, true);
    return hipSuccess;
  }
  void release() {
    if (!h_) return;
    (void)Destroy(h_);
    h_ = nullptr;
    resource_note(KIND, false);
  }

 private:
  H h_ = nullptr;
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy, RES_EVENT>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy, RES_STREAM>;

static_assert(!std::is_copy_constructible<DeviceBuffer>::value && !std::is_copy_assignable<DeviceBuffer>::value, "one owner");
static_assert(!std::is_copy_constructible<PinnedBuffer>::value && !std::is_copy_assignable<PinnedBuffer>::value, "one owner");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value, "one owner");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Stream>::value, "one owner");

}  // namespace vb
