// dp_lm_frame_close.h -- a fragment of text of the LM frame (dp_lm_body.h, dp_clip_rows_body.h), included in place behind
// dp_lm_frame_tangents.h and whatever rows the body added to na: the tiles into the wave's block, then the latent pull.
//   reads      lane, lr16, lk, na, ct, zt and z, the latent whose pass and tangents these were; AB
//   leaves     AB: [J r]^T [J r] with the latent pull, 25 rows of stride SJ -- A = J^T J in rows and columns 0..23, g = J^T r in column 24
//   opens      without a wave_sync(): na is in registers, and AB is read by nobody before the fragment's own
//   closes     with a wave_sync(): AB is every lane's to read
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * mt + 4 * lk + r;
            if (row <= LAT) {
                AB[row * SJ + lr16] = na[mt][0][r];
                AB[row * SJ + 16 + lr16] = na[mt][1][r];
            }
        }
    wave_sync();
    if (lane < LAT) { // the latent pull: sqrt(lambda_tmp / 24) on the diagonal of J, r = that times (z - z_tgt)
        AB[lane * SJ + lane] += ct;
        AB[lane * SJ + LAT] += ct * (z - zt);
    }
    wave_sync();
