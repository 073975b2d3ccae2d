// devmem.h -- the one owner of the library's device and pinned host arrays.
//
// DevArr<T> owns one hipMalloc'd array (PinArr<T>: one hipHostMalloc'd); move-only, empty by default; the destructor, reset() and
// assignment from {} free it.  alloc() refuses an object that already holds an array: captured graphs and kernel plans hold these
// pointers, so nothing is ever re-allocated behind them.  It converts to T* (kernel arguments, pointer arithmetic, null tests read
// as they did on raw pointers).  live_bytes counts what all owners of the process hold.
//
// DEVMEM_HOST_TEST: malloc / free instead of the HIP calls, for the stand-alone check under tools/ (no GPU, sanitizers apply).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

#ifdef DEVMEM_HOST_TEST
#include <cstdlib>
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1;
#else
#include <hip/hip_runtime.h>
#endif

namespace devmem {

inline std::atomic<int64_t> live_bytes{0};

struct Device {
#ifdef DEVMEM_HOST_TEST
    static hipError_t get(void **p, size_t bytes) { *p = std::malloc(bytes ? bytes : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
    static void put(void *p) { std::free(p); }
#else
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void *p) { hipFree(p); }
#endif
};
struct Pinned {
#ifdef DEVMEM_HOST_TEST
    static hipError_t get(void **p, size_t bytes) { return Device::get(p, bytes); }
    static void put(void *p) { Device::put(p); }
#else
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void *p) { hipHostFree(p); }
#endif
};

template <class T, class Where = Device>
class DevArr {
    T     *p_ = nullptr;
    size_t bytes_ = 0;

public:
    DevArr() = default;
    DevArr(DevArr &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevArr &operator=(DevArr &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; bytes_ = o.bytes_;
            o.p_ = nullptr; o.bytes_ = 0;
        }
        return *this;
    }
    ~DevArr() { reset(); }
    void reset() {
        if (p_) { Where::put(p_); live_bytes -= (int64_t)bytes_; }
        p_ = nullptr; bytes_ = 0;
    }
    // exactly n elements (the caller keeps its own convention for empty requests); hipErrorInvalidValue on an object that holds an array
    hipError_t alloc(size_t n) {
        if (p_) return hipErrorInvalidValue;
        void *q = nullptr;
        const hipError_t e = Where::get(&q, n * sizeof(T));
        if (e != hipSuccess || !q) return e;
        p_ = static_cast<T *>(q); bytes_ = n * sizeof(T);
        live_bytes += (int64_t)bytes_;
        return hipSuccess;
    }
    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
};

template <class T> using PinArr = DevArr<T, Pinned>;

} // namespace devmem
