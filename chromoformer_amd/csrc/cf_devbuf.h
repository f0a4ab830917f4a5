// cf_devbuf.h -- DevBuf<T>: the one owner of a device allocation.  Move-only; converts to T*, so launch sites read it as the pointer it
// holds.  Includes the HIP runtime API alone (a stand-alone host program can include it); the includer provides
//     static int fail(const char* fmt, ...);      // records the error text, returns -1
// in front of the #include (cf_api_handle.h does).  No pool, no sub-allocation, no statistics.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <vector>

template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;      // elements

    void release() {
        if (p_) (void)hipFree(p_);      // (synchronises: a call in flight may still read the old buffer)
        p_ = nullptr, cap_ = 0;
    }

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T*() const { return p_; }

    // `count` elements, contents undefined.  What the buffer held is freed FIRST and the pointer nulled: on failure the buffer is empty.
    int alloc(size_t count, const char* who) {
        release();
        void* q = nullptr;
        if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            return fail("%s: out of memory", who);
        }
        p_ = static_cast<T*>(q), cap_ = count;
        return 0;
    }
    // grow-only alloc: at least `count` elements, max(count, floor) when it has to grow; the contents do not survive growing
    int need(size_t count, size_t floor, const char* who) { return count <= cap_ ? 0 : alloc(count > floor ? count : floor, who); }
    // alloc + a synchronous copy from the host
    int upload(const std::vector<T>& v, const char* who) {
        if (alloc(v.size(), who)) return -1;
        if (!v.empty() && hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
            release();
            return fail("%s: upload of %zu bytes failed", who, v.size() * sizeof(T));
        }
        return 0;
    }
};
