"""CPU: the body-part row layout of dp_w4's layer 2 (dragposer_amd/csrc/dp_w4.h, dp_w4_bp.hip).  Block A holds the side-A items,
block B the side-B items, and each block runs only the K-groups of layer 2 its own items touch (7 + 13 instead of 15 + 15).  What
makes that exact: every weight a block leaves out is 0.0 in the folded decoder.  Checked here on the tables the host packs
(dp_debug_pack_w4_bp, dp_debug_pairs_w4_bp), and on the ISA of the new unit."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as G  # noqa: E402

from dragposer_amd import _lib  # noqa: E402
from dragposer_amd.model import DEFAULT_MODEL, HostModel  # noqa: E402

S_L2A, S_L2B, N_GROUPS = 64, 124, 92
NJ, ITEM_DISP, ITEM_VIRT0 = 22, 22, 23
PAIR = np.dtype([("sd", "<f4", (4, 2)), ("mu", "<f4", (4, 2)), ("off", "<f4", (3, 2)), ("sgn", "<f4", 2), ("rho", "<f4", 2),
                 ("item", "<i4", 2), ("kind", "<i4", 2), ("bone_slot", "<i4", 2), ("ch_sub", "<u4", 2), ("pad", "<i4", 2)])
SAVED_MFMAS = 40  # per iteration: (15 - 7) + (15 - 13) K-groups of 4 steps


def _layout():
    items, groups = np.zeros((2, 16), np.int32), np.zeros((2, 15), np.int32)
    assert _lib.load().dp_debug_w4_bp_layout(items.ctypes.data_as(C.c_void_p), groups.ctypes.data_as(C.c_void_p)) == 0
    return items, [g[g >= 0].tolist() for g in groups]


def _pack(hm, bp):
    lib = _lib.load()
    _, folded = hm.fold()
    img, bias = np.zeros((N_GROUPS, 64, 4), np.float32), np.zeros((4, 64), np.float32)
    fn = lib.dp_debug_pack_w4_bp if bp else lib.dp_debug_pack_w4
    rc = fn(C.byref(folded), C.byref(hm.struct), img.ctypes.data_as(C.c_void_p), bias.ctypes.data_as(C.c_void_p))
    return rc, img, bias


def _steps(img, s0, n):
    """[n steps][64 lanes] of the image from step s0"""
    return np.stack([img[(s0 + k) >> 2, :, (s0 + k) & 3] for k in range(n)])


def _virt_parents(parents):
    first, virt = {}, []
    for k in range(1, NJ):
        p = int(parents[k])
        if p == 0:
            continue
        if p in first:
            virt.append(p)
        else:
            first[p] = k
    return virt


def _expected_rows(hm, item):
    """what the kernel's layer 2 computes for `item`: rows sigma * A2 (fp32 of the fp64 product, as the host scales), [4][60]"""
    A2 = hm.fold()[0]["A2"].astype(np.float64)
    virt = _virt_parents(hm.parents)
    out = np.zeros((4, 60), np.float32)
    for c in range(4):
        if item < NJ:
            r, sd = 4 * item + c, float(hm.arrays["std_q"][4 * item + c])
        elif item == ITEM_DISP:
            r, sd = 88 + c, float(hm.arrays["std_disp"][c]) if c < 3 else 0.0
        elif item - ITEM_VIRT0 < len(virt):
            j = virt[item - ITEM_VIRT0]
            r, sd = 4 * j + c, float(hm.arrays["std_q"][4 * j + c])
        else:
            continue
        out[c] = (sd * A2[r]).astype(np.float32)
    return out


@pytest.mark.parametrize("wd", ["fp32", "bf16"])
def test_every_skipped_weight_is_zero_and_the_kept_ones_rebuild_layer2(wd):
    hm = HostModel(DEFAULT_MODEL, weight_dtype=wd)
    rc, img, bias = _pack(hm, bp=True)
    assert rc == 0, _lib.last_error()
    rcd, dimg, dbias = _pack(hm, bp=False)
    assert rcd == 0
    items, groups = _layout()
    assert [len(g) for g in groups] == [7, 13] and all(g[0] == 0 and g == sorted(g) for g in groups)
    for s, s0 in enumerate((S_L2A, S_L2B)):
        kept = _steps(img, s0, 60)  # [step][lane]
        for b in range(16):
            exp = _expected_rows(hm, int(items[s, b])) if items[s, b] >= 0 else np.zeros((4, 60), np.float32)
            for c in range(4):
                row = exp[c].reshape(15, 4)
                skipped = [k for k in range(15) if k not in groups[s]]
                assert np.all(row[skipped] == 0.0), (wd, s, b, c)  # exactly 0.0: leaving them out changes no bit
                got = kept[:, 4 * b + c]
                np.testing.assert_array_equal(got[:4 * len(groups[s])], row[groups[s]].reshape(-1))
                assert np.all(got[4 * len(groups[s]):] == 0.0)
    # everything but layer 2's rows is the dense image, bL2's K order (items 0..25) included
    other = [g for g in range(N_GROUPS) if not S_L2A // 4 <= g < S_L2B // 4 + 15]
    np.testing.assert_array_equal(img[other], dimg[other])
    np.testing.assert_array_equal(bias[:2], dbias[:2])
    # the bias rows: the same per item and channel as the dense layout's (dp_w4.h: item_of, l2_side, l2_channel)
    dense = {}
    for blk in range(2):
        for l in range(64):
            b, r = l >> 2, l & 3
            it = b if r & 1 == 0 else (15 + b if 1 <= b <= 10 else -1)
            dense[(it, 2 * blk + (r >> 1))] = dbias[2 + blk, l]
    for s in range(2):
        for l in range(64):
            it = int(items[s, l >> 2])
            if it >= 0:
                assert bias[2 + s, l] == dense[(it, l & 3)], (s, l)
            else:
                assert tuple(bias[2 + s, l & ~3:(l & ~3) + 4]) == (1.0, 0.0, 0.0, 0.0)  # idle: the unit quaternion


def test_placement_covers_every_item_once_and_keeps_the_root_alone():
    hm = HostModel(DEFAULT_MODEL)
    items, _ = _layout()
    placed = sorted(int(i) for i in items.ravel() if i >= 0)
    assert placed == list(range(26))  # joints, the displacement, three virtual slots
    assert items[0, 0] == 0 and items[1, 0] == -1  # the root's quad: nothing beside it (stage G sums the root table there)
    assert items[0, :9].tolist() == list(range(9))  # bL2's dead-group patterns (items 4, 8 / 1..8) stay side-A quads 1..8
    pairs = np.zeros(16, PAIR)
    assert _lib.load().dp_debug_pairs_w4_bp(C.byref(hm.struct), pairs.ctypes.data_as(C.c_void_p)) == 0
    np.testing.assert_array_equal(pairs["item"].T, items)
    assert pairs["kind"][9, 0] == 2 and not (pairs["kind"][:, 1] == 2).any()  # KIND_DISP on side A only


def test_a_model_whose_skipped_groups_are_not_zero_keeps_the_dense_layout():
    raw = dict(np.load(DEFAULT_MODEL))
    U = raw["decoder.layers.2.0.weight"]  # [92 conv channels][60 hidden]: the 0/1 unpooling
    col = int(np.flatnonzero(U[:, 4 * 8])[0])  # a conv input channel fed by hidden K-group 8 (among others) -- not one of block A's
    W, M = raw["decoder.layers.2.1.weight"].copy(), raw["decoder.layers.2.1.mask"].copy()
    W[1, col, 0], M[1, col, 0] = 0.5, 1.0  # output channel 1 = the root's
    raw["decoder.layers.2.1.weight"], raw["decoder.layers.2.1.mask"] = W, M
    hm = HostModel(arrays=raw)
    rc, _, _ = _pack(hm, bp=True)
    assert rc == _lib.DP_ERR_UNSUPPORTED and "of item 0 is not zero" in _lib.last_error()
    assert _pack(hm, bp=False)[0] == 0


def _kernels(text):
    """{kernel name: (MFMA count, vgpr spills, scratch bytes)} of an assembly listing"""
    notes = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
        notes[name] = (get("vgpr_spill_count"), get("private_segment_fixed_size"))
    parts = re.split(r"^(_Z\w+):[^\n]*$", text, flags=re.M)
    return {n: (b.split(".Lfunc_end")[0].count("v_mfma"),) + notes[n] for n, b in zip(parts[1::2], parts[2::2])}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_body_part_unit_runs_40_mfmas_fewer_per_iteration_without_spills():
    import check_mfma_hazards as H

    dense = _kernels(H.isa([], base_flags=G.HIPCC_FLAGS))
    text = H.isa([], base_flags=G.HIPCC_FLAGS, source="dp_w4_bp.hip")
    bp = _kernels(text)
    assert len(bp) == 6 and all("dp_w4_bp_kernel" in n for n in bp), list(bp)
    for name, (n_mfma, spill, scratch) in bp.items():
        d = dense[name.replace("_Z15dp_w4_bp_kernel", "_Z12dp_w4_kernel")]
        assert n_mfma == d[0] - SAVED_MFMAS, (name, n_mfma, d)  # the loop is unrolled once per instantiation
        assert spill == 0 and scratch == 0, (name, spill, scratch)
    n_mfma, _, bad = H.check(text)
    assert n_mfma == 6 * (452 - SAVED_MFMAS) and not bad, bad[:4]
