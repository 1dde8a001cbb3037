// The host layer's one owning device allocation: a typed pointer + element count that frees itself.  Every device buffer of the
// context is a DeviceBuffer member (or sits in a map / struct of them), so destroying the context releases them all.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace mocha {

enum BufferPolicy : unsigned {
    BUF_PLAIN = 0,
    BUF_MOVES_GENERATION = 1,      // a captured graph may have the pointer baked in: (re)allocating it moves the context generation
    BUF_ZEROED = 2,                // the whole buffer is zero when reserve() hands out a new allocation
};

template <class T>
struct DeviceBuffer {
    T* p = nullptr;
    size_t n = 0;                  // elements
    unsigned policy;               // BufferPolicy bits, stated once where the buffer is declared

    explicit DeviceBuffer(unsigned policy_ = BUF_PLAIN) : policy(policy_) {}
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p), n(o.n), policy(o.policy) { o.p = nullptr; o.n = 0; }
    ~DeviceBuffer() { release(); }

    // waits for earlier work that may still read the allocation, then frees it
    void release() {
        if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); }
        p = nullptr; n = 0;
    }
    // Grow-only: a no-op while `need` elements fit, otherwise the old allocation is released and a new one made (contents are not
    // carried over).  *grew tells the caller that the pointer changed.  On failure the buffer is left empty.
    hipError_t reserve(size_t need, bool* grew = nullptr) {
        if (grew) *grew = false;
        if (n >= need) return hipSuccess;
        release();
        const size_t bytes = std::max<size_t>(need * sizeof(T), 16);
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess && (policy & BUF_ZEROED) && (e = hipMemset(q, 0, bytes)) != hipSuccess) (void)hipFree(q);
        if (e != hipSuccess) return e;
        p = static_cast<T*>(q); n = need;
        if (grew) *grew = true;
        return hipSuccess;
    }
};

}  // namespace mocha
