// buffers.hip.h -- what a handle owns besides the state itself: device scratch, pinned staging, staged uploads.
//
// Released by the destructors, so the owner's teardown names none of them; it must have made the device current and drained
// its streams before the members go.  An empty buffer releases nothing: a planner-only handle makes no HIP call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace qh {

// Device (PINNED = false) or pinned host memory, move-only.  No growth policy and no synchronization: the site passes the
// capacity it wants and drains whatever may still use the old allocation before it asks for more.
template <bool PINNED> struct Buffer {
  void *ptr = nullptr;
  size_t cap = 0;
  Buffer() = default;
  Buffer(Buffer &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Buffer &operator=(Buffer &&o) noexcept {
    std::swap(ptr, o.ptr);
    std::swap(cap, o.cap);
    return *this;
  }
  ~Buffer() { release(); }
  void release() {
    if (ptr) (void)(PINNED ? hipHostFree(ptr) : hipFree(ptr));
    ptr = nullptr;
    cap = 0;
  }
  // at least `bytes`: nothing to do, or release and allocate exactly `bytes`; a failure leaves the buffer empty
  hipError_t reserve(size_t bytes) {
    if (cap >= bytes) return hipSuccess;
    release();
    const hipError_t e = PINNED ? hipHostMalloc(&ptr, bytes, hipHostMallocDefault) : hipMalloc(&ptr, bytes);
    if (e != hipSuccess) {
      ptr = nullptr;
      (void)hipGetLastError();
      return e;
    }
    cap = bytes;
    return hipSuccess;
  }
  template <typename T> T *as() const { return (T *)ptr; }
};
using DeviceBuffer = Buffer<false>;
using PinnedBuffer = Buffer<true>;

// Regions of one scratch buffer: every region starts on a 256-byte boundary, `total` is what to reserve.
struct ScratchLayout {
  size_t total = 0;
  size_t add(size_t bytes) {
    const size_t off = (total + 255) & ~(size_t)255;
    total = off + bytes;
    return off;
  }
};

// Host data on its way to a kernel: the caller fills pinned slot s, copies it into device slot s on its stream, launches
// the reader and commits; slot s is written again only after the event recorded by that commit has completed.  The pinned
// half, the device half and the events exist together or not at all.
template <int N> struct StagedUpload {
  PinnedBuffer host;
  DeviceBuffer dev;
  hipEvent_t ev[N] = {};
  bool used[N] = {};
  unsigned next = 0;
  StagedUpload() = default;
  StagedUpload(const StagedUpload &) = delete;
  StagedUpload &operator=(const StagedUpload &) = delete;
  ~StagedUpload() { release(); }
  void release() {
    for (int i = 0; i < N; ++i) {
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      ev[i] = nullptr;
      used[i] = false;
    }
    host.release();
    dev.release();
  }
  // the event to wait for on the host before acquire() hands out the next slot (nullptr: that slot is free)
  hipEvent_t busy() const { return used[next % N] ? ev[next % N] : nullptr; }
  // The next slot, round-robin, of `bytes_per_slot` each.  A larger size than before reallocates the buffers: with one
  // slot nothing else is in flight once busy() has completed; a ring passes the same size every time.
  hipError_t acquire(size_t bytes_per_slot, char **h, char **d, unsigned *slot) {
    if (host.cap < N * bytes_per_slot || !ev[N - 1]) {
      hipError_t e = host.reserve(N * bytes_per_slot);
      if (e == hipSuccess) e = dev.reserve(N * bytes_per_slot);
      for (int i = 0; i < N && e == hipSuccess; ++i)
        if (!ev[i]) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
      if (e != hipSuccess) {
        release();
        (void)hipGetLastError();
        return e;
      }
    }
    *slot = next++ % N;
    *h = host.template as<char>() + *slot * bytes_per_slot;
    *d = dev.template as<char>() + *slot * bytes_per_slot;
    return hipSuccess;
  }
  // behind the kernel that reads the slot (or behind the copy, when the stream orders the readers)
  hipError_t commit(hipStream_t stream, unsigned slot) {
    const hipError_t e = hipEventRecord(ev[slot], stream);
    used[slot] = e == hipSuccess;
    return e;
  }
};

}  // namespace qh
