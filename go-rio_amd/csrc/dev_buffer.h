// dev_buffer.h -- growable owners of ONE device allocation (DevBuf<T>) or one pinned host allocation (PinnedBuf), and the helper that
// grows several buffers to one shared capacity.  Depends on hip_runtime.h only: no error codes, no fail functions of any module.
//
// The invariant every owner keeps: the capacity is 0 whenever the pointer is null.  A failed allocation therefore leaves an EMPTY buffer
// (never freed pointers, never a capacity without memory behind it), and the next reserve() with any size allocates again.
//
// How much to allocate is the caller's business (reserve(need, grown)): the growth policies differ per site on purpose.  Memory is taken
// with hipMalloc and returned with hipFree, whose implicit device synchronisation is what makes it safe to replace a buffer that
// kernels in flight still read.  Nothing is copied on growth: a site that keeps old contents builds new buffers, copies, and move-assigns.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace gorio {

struct DeviceMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) {
    if (p) (void)hipHostFree(p);
  }
};

template <typename T>
struct buf_elem_size {
  static constexpr size_t value = sizeof(T);
};
template <>
struct buf_elem_size<void> {  // byte buffers
  static constexpr size_t value = 1;
};

template <typename T, typename Mem>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { Mem::release(p_); }  // result ignored: a thread_local owner may die while the HIP runtime is already shutting down

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }  // elements (bytes for T = void)

  void reset() {
    Mem::release(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // Free, then allocate `count` elements.  On failure the buffer is empty and the error comes back.
  hipError_t realloc(size_t count) {
    reset();
    void* p = nullptr;
    const hipError_t e = Mem::alloc(&p, buf_elem_size<T>::value * count);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    cap_ = count;
    return hipSuccess;
  }
  // need <= cap: nothing happens.  Otherwise realloc(grown), grown >= need.
  hipError_t reserve(size_t need, size_t grown) { return need <= cap_ ? hipSuccess : realloc(grown); }
  hipError_t reserve(size_t need) { return reserve(need, need); }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

template <typename T>
using DevBuf = Buf<T, DeviceMem>;
using PinnedBuf = Buf<void, PinnedMem>;

inline void reset_all() {}
template <typename B, typename... Rest>
void reset_all(B& b, size_t, Rest&&... rest) {
  b.reset();
  reset_all(rest...);
}
inline hipError_t realloc_all() { return hipSuccess; }
template <typename B, typename... Rest>
hipError_t realloc_all(B& b, size_t count, Rest&&... rest) {
  const hipError_t e = b.realloc(count);
  return e != hipSuccess ? e : realloc_all(rest...);
}

// Several buffers that grow together behind ONE capacity `cap` (whatever unit the caller counts in): reserve_group(cap, need, grown,
// buf_a, count_a, buf_b, count_b, ...) does nothing while need <= cap; otherwise it frees all of them, then allocates count_x elements
// for each.  Either all of them hold their counts and cap == grown, or all are empty and cap == 0.
template <typename Cap, typename... Bufs>
hipError_t reserve_group(Cap& cap, size_t need, size_t grown, Bufs&&... bufs) {
  if (need <= (size_t)cap) return hipSuccess;
  cap = 0;
  reset_all(bufs...);
  const hipError_t e = realloc_all(bufs...);
  if (e != hipSuccess) {
    reset_all(bufs...);
    return e;
  }
  cap = (Cap)grown;
  return hipSuccess;
}

}  // namespace gorio
