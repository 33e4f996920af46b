// An owning device buffer.  Nothing of hip/ in here: the two free functions are the link-time seam -- engine.hip defines
// them over the HIP allocator, tools/devbuf_check.cpp over malloc -- so that who frees what is checked on the host.
#pragma once
#include <cstddef>

namespace cesx {

// bytes of device memory (never an empty allocation: 0 asks for 8), zeroed when `zero`.  0, or the error of the call
// that failed; nothing stays allocated then, also when it was the memset that failed.
int dev_alloc(void** p, size_t bytes, bool zero);
void dev_free(void* p);

// Move-only.  A buffer that was never allocated (or was moved from, or reset) destructs without a dev_free call.
template <typename T> struct DevBuf {
    T* p = nullptr;
    size_t bytes = 0;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset() {
        if (p) dev_free(p);
        p = nullptr; bytes = 0;
    }
    // what it holds is freed first; a failure (dev_alloc's code) leaves it empty
    int alloc(size_t n, bool zero = true) {
        reset();
        void* q = nullptr;
        if (const int rc = dev_alloc(&q, n, zero)) return rc;
        p = static_cast<T*>(q); bytes = n;
        return 0;
    }
    // kept (contents and all) when it already holds at least n bytes
    int ensure(size_t n, bool zero = true) { return (p && bytes >= n) ? 0 : alloc(n, zero); }
    T* get() const { return p; }
    operator T*() const { return p; }
};

}  // namespace cesx
