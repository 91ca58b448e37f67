// capi_support.h -- what the C ABIs of libvsg_render, libvsg_flow and libvsg_resize share: errors and
// the thread's last error text, device binding, blocks of memory that only grow, the stage clock.
// Include it after the library's public header (VSG_OK, VSG_ERR_*, VSG_MEM_*), from the one
// translation unit that defines the library's entry points.
//
// Everything here is in an unnamed namespace.  The libraries are loaded into one process, and a
// thread-local or a function with vague linkage would be unified across them by the dynamic linker:
// vsg_flow_last_error() would return the renderer's text.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] void Throw(int code, const std::string& msg) { throw Error(code, msg); }

#define VSG_HIP(call)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) Throw(VSG_ERR_DEVICE, std::string(hipGetErrorString(e_)) + " in " #call); \
  } while (0)

thread_local std::string g_last_error;

// The body of an entry point: its status, the text of a failure kept for vsg_X_last_error().
template <class F>
int Guard(F&& f) {
  try {
    f();
    return VSG_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return VSG_ERR_INTERNAL;
  }
}

// Binds the calling thread to the handle's device for the duration of a call (a handle may be
// driven from any thread; the HIP current device is a per-thread setting).
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev_) != hipSuccess) return;
    if (prev_ != device) {
      VSG_HIP(hipSetDevice(device));
      changed_ = true;
    }
  }
  ~DeviceGuard() {
    if (changed_) (void)hipSetDevice(prev_);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;

 private:
  int prev_ = -1;
  bool changed_ = false;
};

void CheckMem(int mem, const char* what) {
  if (mem != VSG_MEM_HOST && mem != VSG_MEM_DEVICE) Throw(VSG_ERR_INVALID, std::string(what) + ": unknown memory kind");
}

// The ordinal a handle is created on: options.device, or the thread's current device for -1.
int SelectDevice(int requested, const char* library) {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    Throw(VSG_ERR_DEVICE, "no usable HIP device (" + (std::string(library) + " has no CPU fallback): ") +
                              (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
  }
  if (requested >= n) Throw(VSG_ERR_DEVICE, "device ordinal out of range");
  int device = requested;
  if (requested < 0) VSG_HIP(hipGetDevice(&device));
  return device;
}

// vsg_X_destroy: the handle's destructor runs on the handle's device, the caller's is restored.
template <class Handle>
void DestroyOnDevice(Handle* h) {
  if (!h) return;
  int prev = -1;
  const bool have = hipGetDevice(&prev) == hipSuccess;
  (void)hipSetDevice(h->device);
  delete h;
  if (have) (void)hipSetDevice(prev);
}

// A device or pinned-host block that only grows; every runtime allocation is counted.  An empty
// block is allocated at exactly the size asked for.
struct Block {
  void* p = nullptr;
  size_t cap = 0;
  bool pinned = false;
  Block() = default;
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() { Release(); }
  void Reserve(size_t bytes, int64_t* allocations) {
    if (bytes <= cap) return;
    Release();
    const size_t want = std::max(bytes, cap + cap / 2);
    if (pinned) VSG_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    else VSG_HIP(hipMalloc(&p, want));
    cap = want;
    ++*allocations;
  }
  void Release() {
    if (!p) return;
    if (pinned) (void)hipHostFree(p);
    else (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* As() const {
    return static_cast<T*>(p);
  }
};

// Times the stages of a call with events on the handle's stream.  The events are created with the
// handle.  A call records them, Begin and then a Mark where each stage ends, and reads them with
// Read after its one synchronisation.
class StageClock {
 public:
  StageClock() = default;
  StageClock(const StageClock&) = delete;
  StageClock& operator=(const StageClock&) = delete;
  ~StageClock() {
    for (hipEvent_t e : events_) {
      if (e) (void)hipEventDestroy(e);
    }
  }
  // events: one for Begin and one for every Mark of the longest call
  void Create(size_t events) {
    events_.assign(events, nullptr);
    stage_.assign(events, 0);
    for (hipEvent_t& e : events_) VSG_HIP(hipEventCreate(&e));
  }
  void Begin(hipStream_t stream) {
    stream_ = stream;
    used_ = 0;
    Mark(0);
  }
  // The work put on the stream since the last Begin or Mark was of this stage.
  void Mark(int stage) {
    if (used_ >= events_.size()) Throw(VSG_ERR_INTERNAL, "event pool exhausted");
    VSG_HIP(hipEventRecord(events_[used_], stream_));
    stage_[used_++] = stage;
  }
  // us[s] = microseconds of stage s since Begin (0 for a stage that did not run).
  void Read(float* us, int stages) const {
    std::fill(us, us + stages, 0.0f);
    for (size_t k = 1; k < used_; ++k) {
      float ms = 0;
      VSG_HIP(hipEventElapsedTime(&ms, events_[k - 1], events_[k]));
      us[stage_[k]] += ms * 1000.0f;
    }
  }

 private:
  hipStream_t stream_ = nullptr;
  std::vector<hipEvent_t> events_;
  std::vector<int> stage_;   // the stage that ended at event k of the running call
  size_t used_ = 0;
};

}  // namespace
