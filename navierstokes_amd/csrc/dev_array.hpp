// dev_array.hpp — who owns device memory: a device array that goes with its owner.  Move-only, freed by its destructor, which is the
// library handles' ONLY release path: a table of DevArrays is dropped by assigning a fresh one (x = {}), which frees at once, member by
// member in the order of declaration — declare a table's arrays in the order they are to be freed in.  (A destructor runs the other
// way round; where the order matters — where the allocations and frees of a handle land moves launch times, profiles/NOTES.md §4.12 —
// the owner's destructor assigns.)  Builders fill a LOCAL table and move it into the handle once it is complete, so a failed build
// leaves the handle as it was.
// Depends on HIP alone (the tools under tools/ include it through spmv_sstream.hpp): every operation returns its hipError_t, and
// capi_internal.hpp puts the MI_* forms on top.  Sizes are exact: n = 0 leaves the array null, which is what the handles' "built?"
// tests read; a caller that wants a floor passes it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

template <hipError_t (*Free)(void*)>
struct HipFree {
    void operator()(void* p) const { (void)Free(p); }
};

template <class T>
struct DevArray {
    std::unique_ptr<T, HipFree<hipFree>> own;
    operator T*() const { return own.get(); }
    T* get() const { return own.get(); }
    hipError_t alloc(size_t n) // n entries, uninitialised
    {
        T* p = nullptr;
        const hipError_t e = hipMalloc(&p, sizeof(T) * n);
        if (e == hipSuccess) own.reset(p);
        return e;
    }
    hipError_t alloc_uncached(size_t n) // ... of uncached memory (the push exchange's receive window); hipFree releases it like any other
    {
        void* p = nullptr;
        const hipError_t e = hipExtMallocWithFlags(&p, sizeof(T) * n, hipDeviceMallocUncached);
        if (e == hipSuccess) own.reset((T*)p);
        return e;
    }
    hipError_t zeros(size_t n) // ... zero-filled, on the NULL stream
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemset(own.get(), 0, sizeof(T) * n);
    }
    hipError_t fill(const T* h, size_t n) const // the first n entries from the host
    {
        return n ? hipMemcpy(own.get(), h, sizeof(T) * n, hipMemcpyHostToDevice) : hipSuccess;
    }
    hipError_t fill(const std::vector<T>& h) const { return fill(h.data(), h.size()); }
    hipError_t upload(const std::vector<T>& h, size_t at_least = 0) // room for h (or at_least entries, if that is more) and h in it
    {
        const hipError_t e = alloc(std::max(h.size(), at_least));
        return e != hipSuccess ? e : fill(h);
    }
};

// pinned host memory that goes with its owner
template <class T>
struct PinnedArray {
    std::unique_ptr<T, HipFree<hipHostFree>> own;
    operator T*() const { return own.get(); }
    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault)
    {
        T* p = nullptr;
        const hipError_t e = hipHostMalloc((void**)&p, sizeof(T) * n, flags);
        if (e == hipSuccess) own.reset(p);
        return e;
    }
};

// a word of host memory that kernels write through dev (the give-up counts of the in-kernel waits: sticky, read by the host at every entry point)
struct MappedWord {
    std::unique_ptr<unsigned, HipFree<hipHostFree>> host;
    unsigned* dev = nullptr;
    hipError_t alloc()
    {
        unsigned* p = nullptr;
        const hipError_t e = hipHostMalloc((void**)&p, sizeof(unsigned), hipHostMallocMapped);
        if (e != hipSuccess) return e;
        host.reset(p);
        *p = 0;
        return hipHostGetDevicePointer((void**)&dev, p, 0);
    }
};

// a stream / an event that goes with its owner; read like the plain handle it replaces
template <class H, hipError_t (*Destroy)(H*)>
struct HipDestroy {
    void operator()(H* h) const { (void)Destroy(h); }
};

struct OwnedStream {
    std::unique_ptr<ihipStream_t, HipDestroy<ihipStream_t, hipStreamDestroy>> own;
    operator hipStream_t() const { return own.get(); }
    hipError_t create(unsigned flags = hipStreamDefault)
    {
        hipStream_t s = nullptr;
        const hipError_t e = flags == hipStreamDefault ? hipStreamCreate(&s) : hipStreamCreateWithFlags(&s, flags);
        if (e == hipSuccess) own.reset(s);
        return e;
    }
};

struct OwnedEvent {
    std::unique_ptr<ihipEvent_t, HipDestroy<ihipEvent_t, hipEventDestroy>> own;
    operator hipEvent_t() const { return own.get(); }
    hipError_t create(unsigned flags = hipEventDefault)
    {
        hipEvent_t ev = nullptr;
        const hipError_t e = flags == hipEventDefault ? hipEventCreate(&ev) : hipEventCreateWithFlags(&ev, flags);
        if (e == hipSuccess) own.reset(ev);
        return e;
    }
};
