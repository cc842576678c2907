// kvazzup_amd/csrc/hip_owner.h -- what one Encoder allocates: device memory, page-locked host memory and events, handed out as the raw pointers and handles
// their users keep as views, and released together.  Every call returns the first HIP error of what it did (callers wrap it in their HIP_OK / HIP_CHECK); a
// pointer that could not be handed out stays as it was.  Under a lock: the lazy sites run on the submitter's and the tokenizer launcher's threads.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>

namespace kvzx {

class HipOwner {
 public:
  ~HipOwner() { release(); }      // (not copyable: the lock)
  template <class T> hipError_t dev(T **p, size_t count, bool zeroed = false)      // count elements of device memory; zeroed: cleared on the null stream
  {
    void *v = nullptr;
    hipError_t e = hipMalloc(&v, count * sizeof(T));
    if (e == hipSuccess) { *p = (T *)v; keep(dev_, v); if (zeroed) e = hipMemset(v, 0, count * sizeof(T)); }
    return e;
  }
  template <class T> hipError_t pinned(T **host, size_t count, unsigned flags, T **alias = nullptr)      // ... of page-locked host memory; alias: where a host-mapped allocation's device address goes
  {
    void *v = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&v, count * sizeof(T), flags);
    if (e == hipSuccess) { *host = (T *)v; keep(host_, v); if (alias && (e = hipHostGetDevicePointer(&d, v, 0)) == hipSuccess) *alias = (T *)d; }
    return e;
  }
  hipError_t event(hipEvent_t *ev, unsigned flags)
  {
    hipError_t e = hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess) keep(ev_, *ev);
    return e;
  }
  void release()      // everything handed out so far; the owner is empty afterwards (a second call does nothing)
  {
    std::lock_guard<std::mutex> l(m_);
    for (void *e : ev_) hipEventDestroy((hipEvent_t)e);
    for (void *p : host_) hipHostFree(p);
    for (void *p : dev_) hipFree(p);
    ev_.clear(); host_.clear(); dev_.clear();
  }
 private:
  void keep(std::vector<void *> &v, void *p) { std::lock_guard<std::mutex> l(m_); v.push_back(p); }
  std::mutex m_; std::vector<void *> dev_, host_, ev_;
};

}  // namespace kvzx
