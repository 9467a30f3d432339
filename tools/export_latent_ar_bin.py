#!/usr/bin/env python3
"""LatentAR -> latent_ar.bin, the flat file libDragPoserDLL.so's drag_poser_load_latent_ar() reads.
Source: the .npz that dragposer_amd.LatentAR.save writes (A [K,24,24], c [24]).  The file holds two tensors, "coeffs" [K,24,24] and
"bias" [24], in that order, as float32.
Format: DPM1 (tools/export_model_bin.py).  Usage: tools/export_latent_ar_bin.py SRC.npz DST"""
import struct
import sys

import numpy as np


def tensors_from(src):
    with np.load(src) as f:
        A, c = np.asarray(f["A"], np.float32), np.asarray(f["c"], np.float32)
    if A.ndim != 3 or A.shape[1:] != (24, 24) or c.shape != (24,):
        raise ValueError(f"{src}: expected A [K,24,24] and c [24], got {A.shape} and {c.shape}")
    return {"coeffs": A, "bias": c}


def write(tensors, dst):
    with open(dst, "wb") as f:
        f.write(b"DPM1" + struct.pack("<I", len(tensors)))
        for k, v in tensors.items():
            a = np.ascontiguousarray(v, dtype=np.float32)
            name = k.encode()
            f.write(struct.pack("<I", len(name)) + name + struct.pack("<I", a.ndim) + struct.pack(f"<{a.ndim}I", *a.shape))
            f.write(a.tobytes())


if __name__ == "__main__":
    write(tensors_from(sys.argv[1]), sys.argv[2])
    print("wrote", sys.argv[2])
