// dp_lm_frame_stage.h -- a fragment of text of the LM frame (dp_lm_body.h, dp_clip_rows_body.h), included in place: where the frame's bones
// stand, and the staging once per workgroup.
//   parameter  FRAME_SKEL 0: the context's bones, staged here at L_OFF;  1: each wave's own [22][3] block skb (filled by dp_lm_frame_skel.h)
//   reads      lds, W, Ti, par, tid, wv
//   leaves     BONES, where the frame's [22][3] bone offsets are read from, by the lane's own off[] and by the tangents, which read another
//              joint's bone (the body #undefs it at its end); with FRAME_SKEL, skb
//   closes     without the barrier: the body's __syncthreads() follows, behind whatever else it stages
#if FRAME_SKEL
#define BONES (skb + wv * SK_W)
    __shared__ float skb[WPB * SK_W]; // [22][3] bones per wave (dp_lm_skel.h)
#else
#define BONES (lds + L_OFF)
#endif
    // ---- staging (once per workgroup): padded weight rows, sigma, the skeleton
    for (int i = tid; i < H0 * LAT; i += WPB * 64) lds[L_A0 + (i / LAT) * S0 + i % LAT] = W[dpvjp::OFF_A0 + i];
    for (int i = tid; i < H1 * H0; i += WPB * 64) lds[L_A1 + (i / H0) * S1 + i % H0] = W[dpvjp::OFF_A1 + i];
    for (int i = tid; i < dpvjp::NY * H1; i += WPB * 64) lds[L_A2 + (i / H1) * S2 + i % H1] = W[dpvjp::OFF_A2 + i];
    if (tid < dpvjp::NY) lds[L_SD + tid] = W[dpvjp::OFF_SD + tid];
    if (tid < NJ) par[tid] = Ti[dpvjp::OFF_PARENT + tid];
#if !FRAME_SKEL
    if (tid < 3 * NJ) lds[L_OFF + tid] = W[dpvjp::OFF_BONE + tid];
#endif
