// dp_host_rt.h -- the host runtime under the C ABI, shared by the three handles (dp_ctx: dp_host.cpp, dp_temporal: dp_temporal_host.cpp,
// dp_encoder: dp_encoder_host.cpp) and the plug-in (dp_unity.cpp: the exception shell only).  Host-only: no device unit includes it.  Every
// hipSetDevice / hipGetDevice / hipMalloc / hipFree / hipHostMalloc / hipHostFree of the host files is in here.  A handle is any struct with
// `int device` and `std::string err`.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/dragposer.h"

namespace dprt {

// ---- error slot: the handle's `err`, or for a NULL handle (a *_create, a host-only packer) the thread-local slot of its family.  A NULL handle
// is passed TYPED (`constexpr dp_ctx* NO_HANDLE = nullptr` in the handle's file): the type names the family.
template <class H>
std::string& null_slot()
{
    static thread_local std::string s;
    return s;
}
template <class H>
int fail(H* h, int code, const std::string& msg)
{
    (h ? h->err : null_slot<H>()) = msg;
    return code;
}
template <class H>
const char* last_error(const H* h) { return h ? h->err.c_str() : null_slot<H>().c_str(); }

// ---- the exception shell: no C++ exception (std::string, std::vector) crosses the C ABI.  A body that throws gives DP_ERR_INVALID with
// "<who>: host-side failure" in the handle's slot -- when even that message cannot be built, the code alone.
template <class H, class Body>
int shell(H* h, const char* who, Body body)
{
    try {
        return body();
    } catch (...) {
        try {
            return fail(h, DP_ERR_INVALID, std::string(who) + ": host-side failure");
        } catch (...) {
            return DP_ERR_INVALID;
        }
    }
}

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

// ---- device selection.  Every entry point that touches the device runs on the handle's device, whatever the calling thread's current device
// is, and leaves the caller's current device as it found it (a NULL stream would otherwise launch on the wrong GPU).  A handle without a
// device (device < 0: dp_debug_host_ctx) makes no runtime call at all and is never `ok`.
struct DeviceGuard : NoCopy {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int device)
    {
        if (device < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = prev == device || hipSetDevice(device) == hipSuccess;
        if (prev == device) prev = -1; // nothing to restore
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The device a *_create is asked for: it exists and is a gfx950 (the library holds gfx950 code objects only).  The refusal goes into H's
// thread-local slot; *n_cu is set when the device reports its compute units.
template <class H>
int open_device(const char* who, int device, int* n_cu)
{
    H* const none = nullptr;
    const std::string w = std::string(who) + ": ";
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(none, DP_ERR_DEVICE, w + "no HIP device (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(none, DP_ERR_INVALID, w + "bad device index");
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(none, DP_ERR_DEVICE, w + "hipGetDeviceProperties: " + hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(none, DP_ERR_DEVICE, w + "device is " + prop.gcnArchName + ", the kernels are built for gfx950 only (no CPU fallback)");
    if (prop.multiProcessorCount > 0) *n_cu = prop.multiProcessorCount;
    return DP_OK;
}

// ---- memory: the four raw calls (dp_io_* hand their results to the caller), and the owners the handles keep theirs in.  An owner frees in
// its destructor, so a handle is deleted under a DeviceGuard of its device; get() is NULL until an upload / alloc has succeeded.
inline hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t device_free(void* p) { return hipFree(p); }
inline hipError_t pinned_alloc(void** p, size_t bytes, unsigned flags = hipHostMallocDefault) { return hipHostMalloc(p, bytes, flags); }
inline hipError_t pinned_free(void* p) { return hipHostFree(p); }

template <class T>
class DeviceBuf : NoCopy {
    T* p_ = nullptr;
    hipError_t alloc(size_t n)
    {
        const hipError_t e = device_alloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }

public:
    ~DeviceBuf() { if (p_) (void)device_free(p_); }
    T* get() const { return p_; }
    hipError_t upload(const std::vector<T>& v) // (once per buffer)
    {
        const hipError_t e = alloc(v.size());
        return e != hipSuccess ? e : hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t alloc_zeroed(size_t n)
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemset(p_, 0, n * sizeof(T));
    }
};

class MappedWord : NoCopy { // one int of page-locked host memory that the device writes and the host reads without a synchronise; starts as 0
    int* p_ = nullptr;

public:
    ~MappedWord() { if (p_) (void)pinned_free(p_); }
    int* get() const { return p_; }
    int read() const { return p_ ? *(volatile const int*)p_ : 0; }
    hipError_t alloc()
    {
        const hipError_t e = pinned_alloc((void**)&p_, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) *p_ = 0;
        else p_ = nullptr;
        return e;
    }
};

} // namespace dprt
