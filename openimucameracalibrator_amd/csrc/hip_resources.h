// Owning holders for what a host entry point takes from the HIP runtime (device memory, pinned host memory, streams, events)
// and the few checks every entry repeats.  Host-side only; DESIGN.md, "Device resources".
//
// THE ORDER RULE.  A holder releases in its destructor, and C++ destroys the locals of a function (and the members of a struct)
// in the reverse order of their declaration.  A buffer may only go once no stream still runs work that reads or writes it, and
// ~Stream waits for its stream before it destroys it.  So: DECLARE A STREAM BEHIND EVERY BUFFER AND EVENT ITS WORK USES, a host
// vector that an asynchronous copy reads or writes included.  Then each return, early or not, first drains the streams and then
// frees the memory; no entry needs a cleanup label or a list of what to free.
// An entry that works on a CALLER's stream owns no Stream: it synchronises that stream itself before its buffers leave scope.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <utility>
#include <vector>
#include "../../include/oicc_hip.h"

namespace oicc {

inline bool hip_ok(hipError_t e) { return e == hipSuccess; }
inline bool hip_ok(bool done) { return done; }
bool hip_ok(int) = delete;      // an OICC_* code is not a hipError_t: compare it yourself
// leaves the entry with OICC_ERR_HIP on a failed runtime call (hipError_t) or holder method (bool); the holders clean up
#define OICC_HIP_TRY(expr) do { if (!oicc::hip_ok(expr)) return OICC_ERR_HIP; } while (0)

inline int select_device(int32_t device_ordinal) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_ordinal < 0 || device_ordinal >= ndev) return OICC_ERR_NO_DEVICE;   // no CPU fallback
  if (hipSetDevice(device_ordinal) != hipSuccess) return OICC_ERR_NO_DEVICE;
  return OICC_OK;
}

// For the entries that launch on a caller's stream: the launch goes to the current device, so the stream (unless it is the null
// stream) and every array have to live there.  OICC_ERR_NO_DEVICE without a device, OICC_ERR_INVALID_ARG for a stranger.
inline int on_current_device(hipStream_t stream, std::initializer_list<const void*> pointers) {
  int ndev = 0, cur = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || hipGetDevice(&cur) != hipSuccess) return OICC_ERR_NO_DEVICE;   // no CPU fallback
  if (stream) {
    hipDevice_t of_stream = 0, of_current = 0;
    if (hipStreamGetDevice(stream, &of_stream) != hipSuccess || hipDeviceGet(&of_current, cur) != hipSuccess || of_stream != of_current) {
      (void)hipGetLastError();
      return OICC_ERR_INVALID_ARG;
    }
  }
  for (const void* p : pointers) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type == hipMemoryTypeUnregistered || (a.type == hipMemoryTypeDevice && a.device != cur)) {
      (void)hipGetLastError();
      return OICC_ERR_INVALID_ARG;
    }
  }
  return OICC_OK;
}

// device buffer that grows on demand
template <class T>
struct DevBuf {
  T* p = nullptr; size_t n = 0;
  bool owned = true;   // false: a piece of a DevArena block
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;              // a copy would free twice
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n), owned(o.owned) { o.p = nullptr; o.n = 0; o.owned = true; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); std::swap(p, o.p); std::swap(n, o.n); std::swap(owned, o.owned); } return *this; }
  ~DevBuf() { if (p && owned) (void)hipFree(p); }
  void release() { if (p && owned) (void)hipFree(p); p = nullptr; n = 0; owned = true; }
  bool resize(size_t count) {
    if (count <= n && p) return true;
    release();
    if (count == 0) return true;
    if (hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)) != hipSuccess) { p = nullptr; return false; }
    n = count; return true;
  }
  bool upload(const T* h, size_t count, hipStream_t st) {   // room for at least one element, so that p is never null afterwards
    if (!resize(std::max<size_t>(count, 1))) return false;
    if (count == 0) return true;
    return hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, st) == hipSuccess;
  }
  bool upload(const std::vector<T>& h, hipStream_t st) { return upload(h.data(), h.size(), st); }
  // copies only, for an entry that has made every allocation ahead of its first copy: count <= n
  bool copy_from(const T* h, size_t count, hipStream_t st) { return hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, st) == hipSuccess; }
  bool copy_from(const std::vector<T>& h, hipStream_t st) { return copy_from(h.data(), h.size(), st); }
  bool download(T* h, size_t count, hipStream_t st) const { return hipMemcpyAsync(h, p, count * sizeof(T), hipMemcpyDeviceToHost, st) == hipSuccess; }
  void attach(T* ptr, size_t count) { release(); p = ptr; n = count; owned = false; }
};

// pinned host memory (staging for asynchronous copies)
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  bool alloc(size_t count) { return !p && hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocDefault) == hipSuccess; }
};

// a non-blocking stream; see THE ORDER RULE above for where to declare one
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { reset(); }
  bool create() { return !s && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess; }
  void reset() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); s = nullptr; } }   // drains first: its work may use buffers that go next
  operator hipStream_t() const { return s; }
};

// For a helper that queues work on its CALLER's stream and owns buffers of its own: declared behind them, it waits for that stream
// on every way out, so that the buffers go only once the stream is through with them.
struct DrainOnExit {
  hipStream_t s;
  ~DrainOnExit() { (void)hipStreamSynchronize(s); }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  bool create() { return !e && hipEventCreate(&e) == hipSuccess; }
  operator hipEvent_t() const { return e; }
};

}  // namespace oicc
