// dp_vjp.h -- layout of the vector-Jacobian product of decode + FK (dp_vjp.hip), shared with the host packer (dp_host.cpp).
//
// One frame per lane, 64 frames per workgroup of one wave; nothing is exchanged between lanes.  The folded decoder runs on the
// VALU with its weights as wave-uniform (scalar-cache) operands; the kinematics keep their per-joint vectors in LDS columns
// private to the lane (the parent of a joint is only known at run time).  Reference of what is differentiated:
// include/dragposer_grad.h.
#pragma once
#include <hip/hip_runtime.h>

namespace dpvjp {

constexpr int NJ = 22, LAT = 24, H0 = 40, H1 = 60, NY = 92;
constexpr int FPB = 64; // frames per workgroup (= lanes of its single wave)

// weight image (floats): the folded decoder (dp_folded: A0 c0 A1 b1 A2 b2, row-major), the de-normalisation of its output
// (sd / mu: 88 quaternion channels, 3 displacement channels, one pad) and the skeleton's bone offsets
constexpr int OFF_A0 = 0;
constexpr int OFF_C0 = OFF_A0 + H0 * LAT;
constexpr int OFF_A1 = OFF_C0 + H0;
constexpr int OFF_B1 = OFF_A1 + H1 * H0;
constexpr int OFF_A2 = OFF_B1 + H1;
constexpr int OFF_B2 = OFF_A2 + NY * H1;
constexpr int OFF_SD = OFF_B2 + NY;
constexpr int OFF_MU = OFF_SD + NY;
constexpr int OFF_BONE = OFF_MU + NY;
// then the skeleton as the kernel walks it (int words): parent of every joint (parent[j] < j), and the children of joint p
// as clist[cstart[p] .. cstart[p + 1])
constexpr int OFF_PARENT = OFF_BONE + 3 * NJ;
constexpr int OFF_CSTART = OFF_PARENT + NJ;
constexpr int OFF_CLIST = OFF_CSTART + NJ + 1;
constexpr int IMG_WORDS = OFF_CLIST + NJ;

struct Args {
    const float* img;     // IMG_WORDS words, packed once per context (dp_create)
    const float* z;       // [B][24]
    const float* cur_rot; // [B][4]
    // upstream gradients, shapes of dp_result's fields; NULL = zero
    const float *g_pose, *g_disp, *g_wdisp, *g_wrot, *g_pos, *g_rot;
    float* dz;   // [B][24]
    float* dcur; // [B][4] or NULL
    int* status; // [B] or NULL
    int n_frames;
};

// dp_vjp_skel_kernel (dp_vjp_skel.hip): the same, with the bones of each frame's own skeleton (include/dragposer_skeleton.h)
struct SkelArgs : Args {
    const float* skel; // [N][22][3]: frame f reads skel + f * skel_stride (rows 1..21)
    int skel_stride;   // 66 (one skeleton per frame) or 0 (one for the launch)
    float* doff;       // [B][22][3] dL/d(offsets) per frame, or NULL
};

} // namespace dpvjp

hipError_t dp_launch_vjp(const dpvjp::Args* args, hipStream_t stream);
hipError_t dp_launch_vjp_skel(const dpvjp::SkelArgs* args, hipStream_t stream);
