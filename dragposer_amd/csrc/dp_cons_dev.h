// dp_cons_dev.h -- device helpers of dp_cons_body.h and the launcher of its kernels, shared by its nine units (dp_cons.hip ..
// dp_cons_points.hip).  Included after the unit's dp_cons*.h, dp_math.h and dp_vjp.h, inside a unit that says `using namespace dpcons;`.
#pragma once

#define DEV __device__ __forceinline__

namespace {

constexpr int NJ = dpvjp::NJ, LAT = dpvjp::LAT, H0 = dpvjp::H0, H1 = dpvjp::H1;
constexpr int NYU = 4 * NJ + 3; // decoder outputs that are used (the 92nd is not)
#ifndef UNR
#define UNR 4 // (the dot products' loops: unrolled further, their loads stay in flight in registers and the frame loop spills)
#endif

DEV void wave_sync()
{ // orders this wave's LDS writes before its later LDS reads (other lanes' data); no instruction
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

DEV float wsum(float x)
{ // sum over lanes 0..31 (every lane that contributes is below 32), result in every lane of the half
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) x += __shfl_xor(x, m, 32);
    return x;
}

DEV float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); } // lane 0's value, wave-uniform

// component `up` of a 3-vector without indexing registers at run time (no scratch)
DEV float comp(const float* v, int up) { return up == 0 ? v[0] : up == 1 ? v[1] : v[2]; }
DEV void flatten(float* v, int up)
{ // h(v): the up component set to 0
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = c == up ? 0.f : v[c];
}

// M v with M row-major 3x3
DEV void mv(const float* M, const float* v, float* o)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = M[3 * r] * v[0] + M[3 * r + 1] * v[1] + M[3 * r + 2] * v[2];
}

// global_pos is read: the floor term is on (four terms) / an active PLANE or point-DISTANCE term exists (table)
DEV bool reads_gp(const Args& a) { return a.w_floor != 0.f; }
DEV bool reads_gp(const TermArgs& a) { return a.need_gp != 0; }

DEV int uni_i(int x) { return __builtin_amdgcn_readfirstlane(x); } // (an int the wave holds in every lane)

// host: what every dp_launch_* of these units does -- a wave per frame (or sequence), WPB waves per workgroup, the argument block by value
template <class A>
hipError_t launch_waves(void (*kernel)(A), const A* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + WPB - 1) / WPB);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(WPB * 64), 0, stream, *args);
    return hipGetLastError();
}

} // namespace
