// Host-only: the one owner of an entry point's scratch device memory.  It keeps the first HIP error it meets (every method is
// a no-op from then on) and the list of what it allocated; the destructor frees all of it - and the stream and events it was
// asked to create - on whichever path the function leaves.  No pool, no cache: what a call allocates, that call frees.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

struct DevScratch {
  hipError_t err;
  std::vector<void*> mem;
  std::vector<hipEvent_t> events;
  hipStream_t own_stream = nullptr;

  explicit DevScratch(int device) : err(hipSetDevice(device)) {}
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() {
    for (hipEvent_t e : events) hipEventDestroy(e);
    if (own_stream) hipStreamDestroy(own_stream);
    for (void* p : mem) hipFree(p);
  }

  bool ok() const { return err == hipSuccess; }

  // n elements, at least one
  template <typename T>
  T* alloc(size_t n) {
    void* p = nullptr;
    if (!ok() || (err = hipMalloc(&p, (n ? n : 1) * sizeof(T))) != hipSuccess) return nullptr;
    mem.push_back(p);
    return (T*)p;
  }
  // a device copy of host[0 .. n), through `st` when one is given; null when there is no host array
  template <typename T>
  T* upload(const T* host, size_t n, hipStream_t st = nullptr) {
    if (!host) return nullptr;
    T* d = alloc<T>(n);
    if (d && n)
      err = st ? hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, st) : hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  void zero(void* p, size_t bytes, hipStream_t st = nullptr) {
    if (ok()) err = st ? hipMemsetAsync(p, 0, bytes, st) : hipMemset(p, 0, bytes);
  }
  // after the launches: their error, then the end of the work on `st` (null: on the device)
  void sync(hipStream_t st = nullptr) {
    if (ok()) err = hipGetLastError();
    if (ok()) err = st ? hipStreamSynchronize(st) : hipDeviceSynchronize();
  }
  void download(void* dst, const void* src, size_t bytes) {
    if (ok() && bytes) err = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  }
  hipStream_t stream() {
    if (ok() && !own_stream) err = hipStreamCreate(&own_stream);
    return own_stream;
  }
  hipEvent_t event() {
    hipEvent_t e = nullptr;
    if (ok() && (err = hipEventCreate(&e)) == hipSuccess) events.push_back(e);
    return e;
  }
};
