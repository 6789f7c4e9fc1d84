// er_devbuf.h -- a device allocation and its element count (host side; er_scene.h `upload` fills one).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace erh {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

template <class T>
struct ScopedDevBuf : DevBuf<T> {   // a temporary: freed on every way out of the function
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf&) = delete;
    ScopedDevBuf& operator=(const ScopedDevBuf&) = delete;
    ~ScopedDevBuf() { this->release(); }
};

}  // namespace erh
