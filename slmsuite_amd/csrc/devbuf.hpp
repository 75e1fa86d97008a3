// One owner type for device memory: what the engine does with a buffer (allocate, allocate zeroed on its stream,
// allocate on first use, let go of it once the stream has drained) and the hipFree nobody has to remember.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace hgs {

// Move-only; frees in its destructor.  Converts to T*, so argument structs and kernel launches take it as the plain
// pointer it wraps.  Every allocating call returns the HIP status and leaves the buffer empty on failure, with the
// runtime's sticky error cleared: the caller decides whether a missing buffer is fatal.
template <typename T> struct DevBuf {
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { free_now(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~DevBuf() { free_now(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }

    // n elements, contents undefined (what was held before is freed first)
    hipError_t alloc(size_t n) {
        free_now();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
        if (e != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); }
        return e;
    }
    // ... zeroed by a memset on `stream`
    hipError_t alloc_zeroed(size_t n, hipStream_t stream) {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemsetAsync(p_, 0, n * sizeof(T), stream);
    }
    // allocate only when empty (buffers made by the first call that needs them)
    hipError_t ensure(size_t n) { return p_ ? hipSuccess : alloc(n); }
    hipError_t ensure_zeroed(size_t n, hipStream_t stream) { return p_ ? hipSuccess : alloc_zeroed(n, stream); }
    // let go of a buffer that launches on `stream` may still use (a buffer about to be regrown)
    hipError_t release(hipStream_t stream) {
        if (!p_) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(stream);
        return e != hipSuccess ? e : free_now();
    }

private:
    hipError_t free_now() {
        T* q = p_;
        p_ = nullptr;
        return q ? hipFree(q) : hipSuccess;
    }
    T* p_ = nullptr;
};

}  // namespace hgs
