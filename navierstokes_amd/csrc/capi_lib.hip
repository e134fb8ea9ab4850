// capi_lib.hip: library, device, cache flush, stream-read probe — part of libmi355spmv.so (see capi_internal.hpp for the layout of the library).
// Built for gfx950 only; no CPU fallback anywhere: every compute entry point needs a HIP device.
#include "capi_internal.hpp"

thread_local std::string g_err;
std::mutex g_mu;

int need_device()
{
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return fail(MI_ERR_NODEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0") +
                                         " (libmi355spmv has no CPU fallback)");
    return MI_OK;
}

// ---------------------------------------------------------------- library
extern "C" int mi_version(void) { return MI355_SPMV_VERSION; }

extern "C" const char* mi_strerror(int status)
{
    switch (status) {
    case MI_OK: return "ok";
    case MI_ERR_ARG: return "invalid argument";
    case MI_ERR_NODEVICE: return "no HIP device (no CPU fallback)";
    case MI_ERR_HIP: return "HIP runtime error";
    case MI_ERR_ALLOC: return "allocation failed";
    case MI_ERR_UNSUPPORTED: return "unsupported";
    case MI_ERR_STATE: return "bad handle state";
    default: return "unknown status";
    }
}

extern "C" const char* mi_last_error(void) { return g_err.c_str(); }

extern "C" int mi_device_count(int* count)
{
    CHECK_ARG(count, "count is null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = (e == hipSuccess) ? c : 0;
    return MI_OK;
}

extern "C" int mi_set_device(int device)
{
    int rc = need_device();
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    return MI_OK;
}

extern "C" int mi_device_synchronize(void)
{
    int rc = need_device();
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return MI_OK;
}

static std::map<int, void*> g_flush;

// read sweep: leaves the caches full of CLEAN lines of a buffer nobody uses
__global__ __launch_bounds__(256) void flush_read_kernel(const double2* __restrict__ p, size_t n16, double* __restrict__ sink)
{
    double s = 0.0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const double2 v = p[i];
        s += v.x + v.y;
    }
    if (s == 123.456) sink[0] = s; // never true: keeps the loads alive
}

static int flush_cache_on(hipStream_t st, bool sync);

extern "C" int mi_flush_cache(void) { return flush_cache_on(nullptr, true); }

extern "C" int mi_flush_cache_async(mi_stream_t s) { return flush_cache_on((hipStream_t)s, false); }

static int flush_cache_on(hipStream_t st, bool sync)
{
    int rc = need_device();
    if (rc) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const size_t bytes = (size_t)512 << 20;
    void* buf = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        void*& slot = g_flush[dev];
        if (!slot) HIP_TRY(hipMalloc(&slot, 2 * bytes + 256));
        buf = slot;
    }
    // Write 512 MiB (as the reference's flush_cache writes its buffer, mpk/utils.cpp:146-154), then READ another 512 MiB:
    // the fill alone would leave the 256 MiB Infinity Cache full of DIRTY lines whose write-back the next kernel then pays
    // for (measured: a cold C4 product 210 us behind the fill alone); behind the read sweep the caches hold clean lines of
    // a buffer nobody uses, i.e. "nothing of the caller's data is cached" and nothing else.
    HIP_TRY(hipMemsetAsync(buf, 1, bytes, st));
    if (!env_is("MI355_FLUSH_FILL_ONLY", "1"))
        hipLaunchKernelGGL(flush_read_kernel, dim3(4096), dim3(256), 0, st, reinterpret_cast<const double2*>((char*)buf + bytes), bytes / 16,
                           reinterpret_cast<double*>((char*)buf + 2 * bytes));
    HIP_TRY(hipGetLastError());
    if (sync) HIP_TRY(hipDeviceSynchronize());
    return MI_OK;
}

// plain read sweep, 16 bytes per lane and step, grid-stride: what this very GPU streams from HBM when nothing else is asked of it
template <bool NT>
__global__ __launch_bounds__(256) void stream_read_kernel(const double2* __restrict__ p, size_t n16, double* __restrict__ sink)
{
    double s = 0.0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        double2 v;
        if (NT) {
            v.x = __builtin_nontemporal_load(&p[i].x);
            v.y = __builtin_nontemporal_load(&p[i].y);
        } else v = p[i];
        s += v.x + v.y;
    }
    if (s == 123.456) sink[0] = s; // never true: keeps the loads alive
}

extern "C" int mi_stream_read_probe(long long bytes, int launches, double* us_per_launch)
{
    CHECK_ARG(bytes >= (1 << 20) && launches >= 1 && us_per_launch, "bad argument");
    int rc = need_device();
    if (rc) return rc;
    LaunchTimer tm;
    DevArray<char> buf;
    HIP_TRY_AS("hipMalloc", buf.alloc((size_t)bytes + 256));
    HIP_TRY(hipMemset(buf, 1, (size_t)bytes + 256));
    if ((rc = tm.init())) return rc;
    double* sink = reinterpret_cast<double*>(buf + ((size_t)bytes / 16) * 16);
    auto launch = [&]() {
        hipLaunchKernelGGL(stream_read_kernel<true>, dim3(2048), dim3(256), 0, nullptr, (const double2*)buf.get(), (size_t)bytes / 16, sink);
        return MI_OK;
    };
    return tm.time(3, launches, launch, us_per_launch);
}
