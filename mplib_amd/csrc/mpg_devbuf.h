// mpg_devbuf.h -- the four move-only owners of HIP resources: DevBuf (device
// memory), PinnedBuf (pinned host memory), Stream, Event.  The only place in
// csrc/ that allocates or releases one (included by mpg_kernels.hip at global
// scope, after the device code, directly before mpg_world.h).
//
// None of them synchronises anything: when a buffer may be replaced (reserve)
// or released (reset, destruction) is the caller's decision.  reserve() keeps
// no contents; it frees the old block before it allocates the new one, of
// exactly n elements, and leaves the buffer empty when the allocation fails.
#pragma once

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_);
      std::swap(cap_, o.cap_);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }  // elements
  hipError_t reserve(size_t n) {
    if (cap_ >= n) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc(&p_, sizeof(T) * n);
    if (e == hipSuccess) cap_ = n;
    else p_ = nullptr;
    return e;
  }
  void reset() {
    if (p_) hipFree(p_);
    p_ = nullptr, cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// hipHostMalloc(flags); dev() is the block as the device sees it (mapped blocks)
constexpr unsigned kPinMapped = hipHostMallocMapped;                             // the host pipeline's ring
constexpr unsigned kPinCoherent = hipHostMallocMapped | hipHostMallocCoherent;  // latency path, server
template <class T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), dev_(o.dev_), cap_(o.cap_) { o.p_ = o.dev_ = nullptr, o.cap_ = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_);
      std::swap(dev_, o.dev_);
      std::swap(cap_, o.cap_);
    }
    return *this;
  }
  ~PinnedBuf() { reset(); }
  T* get() const { return p_; }
  T* dev() const { return dev_; }
  size_t cap() const { return cap_; }  // elements
  hipError_t reserve(size_t n, unsigned flags) {
    if (cap_ >= n) return hipSuccess;
    reset();
    hipError_t e = hipHostMalloc((void**)&p_, sizeof(T) * n, flags);
    if (e != hipSuccess) p_ = nullptr;
    if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer((void**)&dev_, p_, 0);
    if (e == hipSuccess) cap_ = n;
    else reset();
    return e;
  }
  void reset() {
    if (p_) hipHostFree(p_);
    p_ = dev_ = nullptr, cap_ = 0;
  }

 private:
  T *p_ = nullptr, *dev_ = nullptr;
  size_t cap_ = 0;
};

// one handle each; an empty owner holds none
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class HipHandle {
 public:
  HipHandle() = default;
  HipHandle(HipHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  HipHandle& operator=(HipHandle&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(h_, o.h_);
    }
    return *this;
  }
  ~HipHandle() { reset(); }
  hipError_t create(unsigned flags) {
    reset();
    const hipError_t e = Create(&h_, flags);
    if (e != hipSuccess) h_ = nullptr;
    return e;
  }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
  void reset() {
    if (h_) Destroy(h_);
    h_ = nullptr;
  }

 private:
  H h_ = nullptr;
};
using Stream = HipHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using Event = HipHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
