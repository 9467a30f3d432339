// fake_hip.cpp -- what the library's host files (dp_host.cpp, dp_w16_host.cpp, dp_encoder_host.cpp, dp_temporal_host.cpp) link against in the
// stand-alone sanitized host program (main.cpp) instead of the HIP runtime and the kernel units.  No GPU, no HIP library.
//   strict mode (the default): any runtime call aborts -- the code under test is host arithmetic and must not reach the device;
//   fake mode: one gfx950 device, malloc-backed allocations that are counted, memcpy copies, a tracked current device, and "fail the k-th
//   allocation from now".
// The kernel launchers abort in both modes.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dragposer_amd/csrc/dp_cons_skel.h"
#include "../../dragposer_amd/csrc/dp_encoder.h"
#include "../../dragposer_amd/csrc/dp_kernel.h"
#include "../../dragposer_amd/csrc/dp_sequence.h"
#include "../../dragposer_amd/csrc/dp_temporal.h"
#include "../../dragposer_amd/csrc/dp_vjp.h"

namespace {

bool g_fake = false;
int g_current = 0, g_outstanding = 0, g_allocs = 0, g_fail_at = 0;

[[noreturn]] void die(const char* what)
{
    std::fprintf(stderr, "fake_hip: %s called%s\n", what, g_fake ? "" : " in strict mode");
    std::abort();
}
void runtime_call(const char* what)
{
    if (!g_fake) die(what);
}
hipError_t allocate(const char* what, void** p, size_t bytes)
{
    runtime_call(what);
    *p = nullptr;
    if (++g_allocs == g_fail_at) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    ++g_outstanding;
    return hipSuccess;
}
hipError_t release(const char* what, void* p)
{
    runtime_call(what);
    if (p) { std::free(p); --g_outstanding; }
    return hipSuccess;
}

} // namespace

// the controls (declared again in main.cpp)
void fake_hip_mode(bool fake) { g_fake = fake; }
void fake_hip_fail_allocation(int k) { g_allocs = 0; g_fail_at = k; }
int fake_hip_allocations() { return g_allocs; }
int fake_hip_outstanding() { return g_outstanding; }
int fake_hip_current_device() { return g_current; }
void fake_hip_set_current_device(int d) { g_current = d; }

// ---- the fourteen runtime functions the host files reference
hipError_t hipGetDeviceCount(int* n) { runtime_call("hipGetDeviceCount"); *n = 1; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int device) // (the header maps the name to the runtime's versioned symbol)
{
    runtime_call("hipGetDeviceProperties");
    if (device != 0) return hipErrorInvalidDevice;
    std::memset(p, 0, sizeof(*p));
    std::strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
    p->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipGetDevice(int* d) { runtime_call("hipGetDevice"); *d = g_current; return hipSuccess; }
hipError_t hipSetDevice(int d) { runtime_call("hipSetDevice"); g_current = d; return hipSuccess; }
hipError_t hipMalloc(void** p, size_t bytes) { return allocate("hipMalloc", p, bytes); }
hipError_t hipFree(void* p) { return release("hipFree", p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return allocate("hipHostMalloc", p, bytes); }
hipError_t hipHostFree(void* p) { return release("hipHostFree", p); }
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) { runtime_call("hipMemcpy"); std::memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t)
{
    runtime_call("hipMemcpyAsync");
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t bytes) { runtime_call("hipMemset"); std::memset(dst, v, bytes); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { runtime_call("hipDeviceSynchronize"); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { runtime_call("hipStreamSynchronize"); return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory (fake)" : "error (fake)"; }

// ---- the kernel units' exported functions: no launcher is ever reached; the geometry getters answer with placeholders
extern "C" hipError_t dp_launch_w4(const KArgs*, hipStream_t, LaunchPick*) { die("dp_launch_w4"); }
extern "C" hipError_t dp_launch_w4_bp(const KArgs*, hipStream_t, LaunchPick*) { die("dp_launch_w4_bp"); }
extern "C" hipError_t dp_launch_w4sk(const KArgs*, hipStream_t, LaunchPick*) { die("dp_launch_w4sk"); }
extern "C" hipError_t dp_launch_w4sk_bp(const KArgs*, hipStream_t, LaunchPick*) { die("dp_launch_w4sk_bp"); }
extern "C" hipError_t dp_launch_w16(const KArgs*, hipStream_t, int, LaunchPick*) { die("dp_launch_w16"); }
extern "C" hipError_t dp_launch_sequence_advance(const SeqArgs*, hipStream_t) { die("dp_launch_sequence_advance"); }
extern "C" hipError_t dp_launch_sequence_history(const HistArgs*, hipStream_t) { die("dp_launch_sequence_history"); }
hipError_t dp_launch_vjp(const dpvjp::Args*, hipStream_t) { die("dp_launch_vjp"); }
hipError_t dp_launch_vjp_skel(const dpvjp::SkelArgs*, hipStream_t) { die("dp_launch_vjp_skel"); }
hipError_t dp_launch_cons(const dpcons::Args*, hipStream_t) { die("dp_launch_cons"); }
hipError_t dp_launch_terms(const dpcons::TermArgs*, hipStream_t) { die("dp_launch_terms"); }
hipError_t dp_launch_cons_skel(const dpcons::SkelArgs*, hipStream_t) { die("dp_launch_cons_skel"); }
hipError_t dp_launch_terms_skel(const dpcons::TermSkelArgs*, hipStream_t) { die("dp_launch_terms_skel"); }
int dpenc::launch_encoder(const EncArgs&, int, void*) { die("launch_encoder"); }
hipError_t dpt::dp_launch_temporal(int, int, int, const TArgs&, hipStream_t) { die("dp_launch_temporal"); }
extern "C" int dp_w4_lds_bytes(void) { return 0; }
extern "C" int dp_w4_frames_per_block(void) { return 16; }
extern "C" int dp_w16_lds_bytes(void) { return 0; }
extern "C" int dp_w16_frames_per_wave(void) { return 16; }
int dpt::dp_temporal_team_blocks_per_cu() { runtime_call("dp_temporal_team_blocks_per_cu"); return 1; }
int dpt::dp_temporal_stream_cus(hipStream_t, int n_cu) { runtime_call("dp_temporal_stream_cus"); return n_cu; }
