"""NumPy emulation of dp_encoder.hip: walks the kernel's weight image (dp_debug_encoder_image) in the kernel's own tile and K-step
order with the MFMA's lane maps, so a packer / lane-map / K-order error shows without a GPU.  The constants restate
dragposer_amd/csrc/dp_encoder.h on purpose (a second statement of the layout, not an import of it).

v_mfma_f32_16x16x4_f32 (A = weights, B = poses): lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][pose l & 15]; register r of
lane l of the result is row 4 (l >> 4) + r of pose l & 15; the sum over k is an fp32 multiply-add chain in k order starting from C."""
import numpy as np

TILES = (7, 5, 3, 3)
STEPS = (44, 28, 20, 12)
W_OFF = tuple(int(sum(TILES[i] * STEPS[i] * 64 for i in range(l))) for l in range(4))
B_OFF = tuple(int(sum(TILES[i] * STEPS[i] * 64 for i in range(4)) + sum(16 * TILES[i] for i in range(l))) for l in range(4))
IMG_WORDS = B_OFF[3] + 16 * TILES[3]


def _fma(a, b, c):
    """fp32 fused multiply-add through fp64 (the product of two fp32 values is exact there)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _w_word(l, t, s, lane):
    return W_OFF[l] + ((t * (STEPS[l] // 4) + (s >> 2)) * 64 + lane) * 4 + (s & 3)


def emulate(image, pose, eps=None):
    """image [IMG_WORDS] fp32, pose [n,176] fp32, eps [n,24] or None -> mu, logvar, latent [n,24] fp32"""
    image = np.asarray(image, np.float32)
    pose = np.asarray(pose, np.float32)
    n = pose.shape[0]
    rows16 = np.arange(16)
    # layer 0's B operands: K step s = (j, c) is component c of the lane's j-th 16-byte load, lane group g loading channels 16 j + 4 g ..
    x = [np.stack([pose[:, 16 * (s >> 2) + 4 * g + (s & 3)] for g in range(4)]) for s in range(STEPS[0])]  # [steps][k = g][pose]
    for l in range(4):
        acc = []
        for t in range(TILES[l]):
            c = image[B_OFF[l] + 16 * t + rows16]  # register r of lane group g = bias word 16 t + 4 g + r = row m = 4 g + r
            acc.append(np.repeat(c[:, None], n, axis=1).astype(np.float32))
        for s in range(STEPS[l]):  # the kernel runs the tiles of a step side by side; a tile's own chain is in step order
            for t in range(TILES[l]):
                for k in range(4):
                    a_col = image[[_w_word(l, t, s, 16 * k + m) for m in range(16)]]
                    acc[t] = _fma(a_col[:, None], x[s][k][None, :], acc[t])
        if l < 3:  # register r of tile t on lane group g becomes the B operand of step 4 t + r, k = g
            act = [np.where(a > 0, a, np.float32(0.2) * a).astype(np.float32) for a in acc]
            x = [np.stack([act[s >> 2][4 * g + (s & 3)] for g in range(4)]) for s in range(4 * TILES[l])]
    mu = np.empty((n, 24), np.float32)
    lv = np.empty((n, 24), np.float32)
    mu[:, :16], lv[:, :16] = acc[0].T, acc[1].T
    for g in range(4):
        for r in range(4):
            dst = mu if g % 2 == 0 else lv
            dst[:, 16 + 4 * (g >> 1) + r] = acc[2][4 * g + r]
    latent = mu.copy() if eps is None else (mu + np.asarray(eps, np.float32) * np.exp(np.float32(0.5) * lv)).astype(np.float32)
    return mu, lv, latent
