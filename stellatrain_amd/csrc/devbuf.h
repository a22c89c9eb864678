// devbuf.h -- an owning, grow-only device buffer.
//
// Every device allocation the host layer owns is a DevBuf<T>: the pointer and
// the capacity it backs travel together, the destructor frees, and the one way
// to size it is reserve().  The invariant, after every call whatever it
// returned: get() == nullptr exactly when cap() == 0.  A failed reserve()
// leaves the buffer empty, so the next reserve() allocates again; a capacity
// never outlives the memory behind it.
//
// reserve(need, stream, zero, &fresh, limit):
//   need <= cap()   nothing happens (no wait, no call), *fresh = false.
//   otherwise       the stream's in-flight work (which may still read the old
//                   block) is waited for, the old block is freed, and
//                   min(limit, max(need, cap + cap / 2)) elements are
//                   allocated; with `zero` the whole new capacity is zeroed by
//                   a hipMemsetAsync on that stream.  *fresh = true: the
//                   memory is new, whatever the caller kept in the old block
//                   (tags, counts) is gone.
// The caller keeps need <= limit.  Only the HIP runtime API is used, so host
// compilers take this header and a test can stand in for the five calls.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>

namespace stg {

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_;
            cap_ = o.cap_;
            o.p_ = nullptr;
            o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    T *get() const { return p_; }
    size_t cap() const { return cap_; }  // elements

    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }

    hipError_t reserve(size_t need, hipStream_t stream, bool zero, bool *fresh = nullptr, size_t limit = ~size_t(0)) {
        if (fresh) *fresh = false;
        if (need <= cap_) return hipSuccess;
        const size_t n = std::min(limit, std::max(need, cap_ + cap_ / 2));
        hipError_t e = hipStreamSynchronize(stream);
        release();
        if (e != hipSuccess) return e;
        void *q = nullptr;
        if ((e = hipMalloc(&q, n * sizeof(T))) != hipSuccess) return e;
        if (zero && (e = hipMemsetAsync(q, 0, n * sizeof(T), stream)) != hipSuccess) {
            (void)hipFree(q);
            return e;
        }
        p_ = static_cast<T *>(q);
        cap_ = n;
        if (fresh) *fresh = true;
        return hipSuccess;
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

}  // namespace stg
