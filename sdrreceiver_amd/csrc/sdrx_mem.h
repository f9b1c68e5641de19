// sdrx_mem.h -- who owns device and pinned host memory: Owned<T, Mem>, a move-only typed pointer with its element count.  The
// one place that knows how a buffer of libsdrx is obtained, cleared, grown, sized and released; a context and a group hold
// their memory in these and in nothing else.  `Mem` names the memory functions (error type, ok, obtain, clear, release): HIP's
// for the library (DevBuf / PinBuf below, with hipcc only), a counting fake for host/mem_check.cpp -- apart from the HIP
// policies the header is plain C++.
#pragma once

#include <cstddef>

namespace sdrx {

template <class T, class Mem>
class Owned {
  public:
    using error = typename Mem::error;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~Owned() { reset(); }

    // `count` elements in place of whatever is held (released first), cleared with `zero` (synchronously).  On failure: empty.
    error alloc(size_t count, bool zero = false)
    {
        reset();
        void *p = nullptr;
        error e = Mem::obtain(&p, count * sizeof(T));
        if (e == Mem::ok && zero && (e = Mem::clear(p, count * sizeof(T))) != Mem::ok)
            Mem::release(p);
        if (e != Mem::ok)
            return e;
        p_ = static_cast<T *>(p), n_ = count;
        return e;
    }
    // Grow-only: nothing if `count` elements fit; else release, then obtain (the peak is the larger buffer, not both; the
    // contents are not kept).  On failure: empty, capacity 0.
    error reserve(size_t count) { return count <= n_ ? Mem::ok : alloc(count); }
    void reset()
    {
        if (p_)
            Mem::release(p_);
        p_ = nullptr, n_ = 0;
    }

    T *get() const { return p_; }
    operator T *() const { return p_; } // (kernels and copies take raw pointers)
    size_t count() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }

  private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

#ifdef __HIPCC__
struct HipDevice {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error obtain(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static error clear(void *p, size_t bytes) { return hipMemset(p, 0, bytes); }
    static void release(void *p) { (void)hipFree(p); }
};
struct HipPinned {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error obtain(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static error clear(void *p, size_t bytes) { return memset(p, 0, bytes), hipSuccess; }
    static void release(void *p) { (void)hipHostFree(p); }
};
template <class T>
using DevBuf = Owned<T, HipDevice>;
template <class T>
using PinBuf = Owned<T, HipPinned>;
#endif

} // namespace sdrx
