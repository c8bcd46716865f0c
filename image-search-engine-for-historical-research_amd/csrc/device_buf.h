// Owning device buffers of the handles (api_*.hip).  A DeviceBuf<T> member IS the buffer: it frees its memory when it is reset or
// destroyed, it knows its size, and one constructed on a DeviceBufSet is reached by that set's bytes() and reset() -- which is
// what a handle's hbm_bytes sums and what its destroy frees -- so the struct field is the only place a buffer is named.
// Host code only.  Included by api_internal.h behind the HIP runtime, device_malloc (hipMalloc with one retry), fail and the
// MI_* codes; a program that supplies stand-ins for those can include it alone (tests/device_buf_check.cpp).
#pragma once
#include <cstddef>
#include <string>

// elements allocated for a request of `count`: a quarter of spare, so that a slowly growing request does not reallocate every call
static inline size_t grow_capacity(size_t count) { return count + count / 4 + 64; }

class DeviceBufBase;
// the buffers of one handle, linked as they are constructed.  Declared BEFORE them in the handle, so that it outlives them
struct DeviceBufSet {
  DeviceBufBase* head = nullptr;
  inline size_t bytes() const;       // allocated bytes of every buffer
  inline void reset();               // frees every buffer
};

class DeviceBufBase {
 public:
  DeviceBufBase(const DeviceBufBase&) = delete;
  DeviceBufBase& operator=(const DeviceBufBase&) = delete;
  size_t bytes() const { return bytes_; }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }

 protected:
  explicit DeviceBufBase(DeviceBufSet* set) {
    if (set) next_ = set->head, set->head = this;
  }
  ~DeviceBufBase() { reset(); }
  // the memory moves, the place in a set does not: each object stays in the set it was constructed on
  void take(DeviceBufBase& o) {
    reset();
    p_ = o.p_, bytes_ = o.bytes_;
    o.p_ = nullptr, o.bytes_ = 0;
  }
  // frees, then allocates exactly `bytes`; empty on failure
  hipError_t alloc_bytes(size_t bytes) {
    reset();
    const hipError_t e = device_malloc(&p_, bytes);
    if (e == hipSuccess) bytes_ = bytes;
    else p_ = nullptr;
    return e;
  }
  static int alloc_failed(hipError_t e, size_t bytes) {
    return fail(e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP,
                "device buffer of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
  }
  void* p_ = nullptr;
  size_t bytes_ = 0;

 private:
  friend struct DeviceBufSet;
  DeviceBufBase* next_ = nullptr;
};

inline size_t DeviceBufSet::bytes() const {
  size_t b = 0;
  for (const DeviceBufBase* x = head; x; x = x->next_) b += x->bytes();
  return b;
}
inline void DeviceBufSet::reset() {
  for (DeviceBufBase* x = head; x; x = x->next_) x->reset();
}

template <typename T>
class DeviceBuf : public DeviceBufBase {
 public:
  DeviceBuf() : DeviceBufBase(nullptr) {}
  explicit DeviceBuf(DeviceBufSet& set) : DeviceBufBase(&set) {}
  explicit DeviceBuf(DeviceBufSet* set) : DeviceBufBase(set) {}      // NULL: in no set
  DeviceBuf(DeviceBuf&& o) noexcept : DeviceBufBase(nullptr) { take(o); }
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {
    if (this != &o) take(o);
    return *this;
  }
  T* get() const { return static_cast<T*>(p_); }
  operator T*() const { return get(); }
  size_t count() const { return bytes_ / sizeof(T); }

  // exactly `count` elements, whatever was there before (primary storage sized once at creation)
  hipError_t alloc(size_t count) { return alloc_bytes(count * sizeof(T)); }
  // at least `count` elements: nothing happens when they are there; otherwise the buffer is freed, then `want` elements are
  // allocated.  Contents are not kept.  A failed allocation leaves the buffer empty
  int ensure(size_t count, size_t want) {
    if (p_ && this->count() >= count) return MI_OK;
    const hipError_t e = alloc(want);
    return e == hipSuccess ? (int)MI_OK : alloc_failed(e, want * sizeof(T));
  }
  int grow(size_t count) { return ensure(count, grow_capacity(count)); }
  int grow_exact(size_t count) { return ensure(count, count); }      // no slack: what is allocated is what was asked for
  // grow() whose first `keep` elements survive: the new block is allocated and filled before the old one is freed
  int grow_keep(size_t count, size_t keep) {
    if (p_ && this->count() >= count) return MI_OK;
    const size_t want = grow_capacity(count) * sizeof(T);
    void* q = nullptr;
    hipError_t e = device_malloc(&q, want);
    if (e != hipSuccess) {
      reset();
      return alloc_failed(e, want);
    }
    if (keep && p_ && (e = hipMemcpy(q, p_, keep * sizeof(T), hipMemcpyDeviceToDevice)) != hipSuccess) {
      (void)hipFree(q);
      return fail(MI_ERR_HIP, std::string("device buffer copy: ") + hipGetErrorString(e));
    }
    reset();
    p_ = q, bytes_ = want;
    return MI_OK;
  }
};

// several buffers that hold one entry per result (ids, scores, ...): grown together, each with its own count
template <typename... B>
static int grow_all(size_t count, B&... b) {
  int rc = MI_OK;
  (void)(((rc = b.grow(count)) == MI_OK) && ...);
  return rc;
}
