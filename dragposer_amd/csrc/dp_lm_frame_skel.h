// dp_lm_frame_skel.h -- a fragment of text of the LM frame with a skeleton of its own (FRAME_SKEL 1 of dp_lm_frame_stage.h), included in place
// with the frame's other loads: lane j takes row j of the skeleton into the wave's own block.  One unconditional load per row, the lanes beyond
// the joints on the last row; what is no bone (row 0, those lanes) is selected away afterwards.  A component out of range refuses the frame
// (include/dragposer_skeleton.h's rule).
//   parameter  FRAME_SKEL_ROW  the row's offset in a.skel, in floats (stride 0: the launch's one skeleton)
//   reads      a.skel, lane's j and jl, BONES
//   leaves     bsk, the lane's part of the frame's screening; BONES[3 j + c] written, read by the same lane before any wave_sync() and by
//              the others behind the pass's
    bool bsk = false;
    {
        const float* __restrict__ sk = a.skel + FRAME_SKEL_ROW + 3 * (jl ? j : NJ - 1);
        float o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = sk[c];
        const bool bone = jl && j != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) bsk = bsk || (bone && refused(o[c]));
        if (jl)
#pragma unroll
            for (int c = 0; c < 3; ++c) BONES[3 * j + c] = bone ? o[c] : 0.f;
    }
