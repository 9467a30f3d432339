#!/usr/bin/env python3
"""BVH motion clips -> tests/golden/<name>.npz, the compact exact form __graft_entry__.unpack_clip turns back into the same bytes.
Used once for the reference's three motion files (python/data/example/eval/example{,_2,_3}.bvh, CC BY-SA 4.0):

    python tools/pack_clips.py <dir>/example.bvh <dir>/example_2.bvh <dir>/example_3.bvh [--out tests/golden]

A clip must have the regular layout unpack_clip rebuilds (every MOTION value printed as %.6f, each row ending in " \\n"); the
packed file is unpacked again and compared byte for byte before it is written."""
import argparse
import hashlib
import io
import lzma
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import unpack_clip  # noqa: E402


def pack(data):
    k = data.index(b"\n", data.index(b"Frame Time:")) + 1  # the last header line
    rows = data[k:].decode().split("\n")
    if rows[-1] != "" or any(not r.endswith(" ") for r in rows[:-1]):
        raise ValueError("every MOTION row must end in ' \\n'")
    toks = [r[:-1].split(" ") for r in rows[:-1]]
    v = np.array([[int(t.replace(".", "")) for t in r] for r in toks], dtype=np.int64)  # (%.6f checked by the round trip below)
    negzero = np.array([i for i, t in enumerate(t for r in toks for t in r) if t == "-0.000000"], dtype=np.int64)
    r = np.diff(np.diff(v, axis=0, prepend=0), axis=0, prepend=0)
    if np.abs(r).max() >= 2 ** 31:
        raise ValueError("second differences do not fit 32 bits")
    u = ((r << 1) ^ (r >> 63)).astype("<u4")  # zigzag
    planes = np.ascontiguousarray(np.ascontiguousarray(u.T).view(np.uint8).reshape(-1, 4).T)  # byte planes, channel-major
    return dict(head=np.frombuffer(data[:k], np.uint8), shape=np.array(v.shape, np.int64), negzero=negzero,
                planes=np.frombuffer(lzma.compress(planes.tobytes(), preset=9 | lzma.PRESET_EXTREME), np.uint8),
                sha256=np.frombuffer(hashlib.sha256(data).hexdigest().encode(), np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("bvh", nargs="+")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    for src in args.bvh:
        data = open(src, "rb").read()
        buf = io.BytesIO()
        np.savez(buf, **pack(data))  # (uncompressed: `planes` is compressed already)
        dst = os.path.join(args.out, os.path.basename(src) + ".npz")
        tmp = dst + ".tmp.npz"
        with open(tmp, "wb") as f:
            f.write(buf.getvalue())
        if unpack_clip(tmp) != data:
            os.remove(tmp)
            raise SystemExit(f"{src}: the packed form does not reproduce the file")
        os.replace(tmp, dst)
        print(f"wrote {dst}: {len(buf.getvalue())} bytes for {len(data)}")


if __name__ == "__main__":
    main()
