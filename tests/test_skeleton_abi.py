"""CPU: the per-frame-skeleton entry points of include/dragposer_skeleton.h -- header, binding, exports, argument checks, the rule by which
the kernel picks a lane's bone rows (against the host's own tables), the coverage table of the new kernels and their register budget.  No
compute call is made here (the GPU side is tests/test_hip_skeleton.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import __graft_entry__ as G
from dragposer_amd import _lib
from dragposer_amd.model import DEFAULT_MODEL, HostModel
from skeleton_cases import SKEL_INSTANTIATIONS, skel_symbol  # tests/skeleton_cases.py
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)
from test_hip_topology import TREES  # (the two other trees the GPU tests use)
from test_w4_bp_layout import PAIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_skeleton.h")
NJ, SLOT_TRASH, MAX_ROOT_CH = 22, 24, 3
ITEM = np.dtype([("sd", "f4", 4), ("mu", "f4", 4), ("ch_off", "f4", 3), ("ch_id", "i4"), ("ch_sub", "u4"), ("path_lo", "u4"), ("path_hi", "u4"),
                 ("src_quad", "i4"), ("dst_quad", "i4"), ("kind", "i4"), ("init_id", "i4"), ("init_off", "f4", 3), ("pad", "i4", 10)])


def test_header_declares_the_skeleton_symbols_and_the_library_exports_them():
    text = open(HDR).read()
    declared = set(re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M))
    assert declared == set(_lib.SKELETON_SYMBOLS)
    assert not set(_lib.SKELETON_SYMBOLS) & set(_lib.PUBLIC_SYMBOLS)  # (dragposer.h declares nothing new)
    assert "DP_KERNEL_W16" in text and "DP_ERR_UNSUPPORTED" in text and "8192" in text  # the refusal and the price of AUTO are stated
    lib = _lib.load()
    for sym in declared:
        assert hasattr(lib, sym), sym
    for src in ("dp_w4_skel.hip", "dp_w4_bp_skel.hip"):
        assert src in G.HIP_SOURCES and src in G.W4_UNITS  # (built, and held to the MFMA hazard walk with its own fallback)


def test_skeleton_in_layout_matches_the_c_compiler(tmp_path):
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.DpSkeletonIn) == 8 + ptr + 8
    if shutil.which("gcc") is None:
        pytest.skip("no gcc: layout checked against the arithmetic above only")
    fields = ("struct_size", "reserved0", "offsets", "stride")
    src = tmp_path / "skel.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_skeleton.h"\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(dp_skeleton_in));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_skeleton_in, {f}));\n' for f in fields)
                   + 'dp_skeleton_in s = DP_SKELETON_IN_INIT; printf("%u %d %d\\n", s.struct_size, (s.offsets != 0) + (int)s.reserved0 + s.stride, '
                   'DP_SKELETON_STRIDE);\nreturn 0; }\n')
    exe = tmp_path / "skel"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = subprocess.check_output([str(exe)]).decode().split()
    want = [str(C.sizeof(_lib.DpSkeletonIn))] + [str(getattr(_lib.DpSkeletonIn, f).offset) for f in fields] + [str(C.sizeof(_lib.DpSkeletonIn)),
                                                                                                              "0", str(_lib.DP_SKELETON_STRIDE)]
    assert got == want


def _host_ctx(lib):
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK and ctx.value  # a context with no device behind it
    return ctx


def test_argument_errors_are_refused_before_any_device_is_touched():
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p).value
    batch = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    params = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
    res = _lib.DpResult()
    good = _lib.DpSkeletonIn(offsets=p, stride=66)
    rc = lib.dp_optimize_skeleton(None, C.byref(batch), C.byref(params), C.byref(good), C.byref(res), None)
    assert rc == _lib.DP_ERR_INVALID and b"ctx is NULL" in lib.dp_last_error(None)
    ctx = _host_ctx(lib)
    try:
        def opt(sk, pr=params):
            return lib.dp_optimize_skeleton(ctx, C.byref(batch), C.byref(pr), sk, C.byref(res), None), lib.dp_last_error(ctx).decode()

        def fwd(sk):
            return lib.dp_forward_skeleton(ctx, 4, p, p, sk, C.byref(res), None), lib.dp_last_error(ctx).decode()

        for call in (opt, fwd):
            rc, msg = call(None)
            assert rc == _lib.DP_ERR_INVALID and "skeleton is NULL" in msg, call
            rc, msg = call(C.byref(_lib.DpSkeletonIn(stride=66)))
            assert rc == _lib.DP_ERR_INVALID and "offsets is NULL" in msg, call
            for stride in (1, 3, 65, 67, -66, 132):
                rc, msg = call(C.byref(_lib.DpSkeletonIn(offsets=p, stride=stride)))
                assert rc == _lib.DP_ERR_INVALID and "stride" in msg, (call, stride)
            for size, rsv in ((0, 0), (8, 0), (C.sizeof(good) - 5, 0), (5000, 0), (C.sizeof(good), 3)):
                bad = _lib.DpSkeletonIn(offsets=p, stride=66)
                bad.struct_size, bad.reserved0 = size, rsv
                rc, msg = call(C.byref(bad))
                assert rc == _lib.DP_ERR_INVALID and "struct_size" in msg, (call, size, rsv)
            for stride in (0, 66):  # well-formed: refused only because there is no device
                rc, msg = call(C.byref(_lib.DpSkeletonIn(offsets=p, stride=stride)))
                assert rc == _lib.DP_ERR_DEVICE, (call, stride, rc, msg)
        w16 = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0, kernel=_lib.DP_KERNEL_W16)
        rc, msg = opt(C.byref(good), w16)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "DP_KERNEL_W16" in msg
        for k in (_lib.DP_KERNEL_AUTO, _lib.DP_KERNEL_W4):
            pk = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0, kernel=k)
            assert opt(C.byref(good), pk)[0] == _lib.DP_ERR_DEVICE
        # the sequence entry point: the same refusals, after dp_optimize_sequence's own checks
        fr = _lib.DpSeqFrames(n_steps=2, tgt_pos=p, tgt_rot=p, w=p, tracked=p, z_tgt=p)
        st = _lib.DpSeqState(global_pos=p, global_rot=p, latent_buf=p, disp_buf=p, heights_buf=p, history=4, n_heights=1)
        sr = _lib.DpSeqResults(hist_scratch=p)

        def seq(sk, pr=params):
            rc = lib.dp_optimize_sequence_skeleton(ctx, 4, p, C.byref(fr), C.byref(pr), sk, C.byref(st), None, C.byref(sr), None)
            return rc, lib.dp_last_error(ctx).decode()

        assert seq(None) == (_lib.DP_ERR_INVALID, "dp_optimize_sequence_skeleton: the skeleton is NULL")
        rc, msg = seq(C.byref(_lib.DpSkeletonIn(offsets=p, stride=22)))
        assert rc == _lib.DP_ERR_INVALID and "stride" in msg
        rc, msg = seq(C.byref(good), w16)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "DP_KERNEL_W16" in msg
        assert seq(C.byref(good))[0] == _lib.DP_ERR_DEVICE
    finally:
        lib.dp_destroy(ctx)


def test_the_plain_entry_points_refuse_a_context_without_a_device_image():
    """dp_optimize, dp_forward and dp_optimize_sequence, like the calls above: a well-formed call on a context that has no device image is
    refused with DP_ERR_DEVICE after every argument check (the kernel selector included), before anything of the image is read"""
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p).value
    batch = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    params = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
    res = _lib.DpResult()
    fr = _lib.DpSeqFrames(n_steps=2, tgt_pos=p, tgt_rot=p, w=p, tracked=p, z_tgt=p)
    st = _lib.DpSeqState(global_pos=p, global_rot=p, latent_buf=p, disp_buf=p, heights_buf=p, history=4, n_heights=1)
    sr = _lib.DpSeqResults(hist_scratch=p)
    ctx = _host_ctx(lib)
    try:
        calls = {"dp_optimize": lambda: lib.dp_optimize(ctx, C.byref(batch), C.byref(params), C.byref(res), None),
                 "dp_forward": lambda: lib.dp_forward(ctx, 4, p, p, C.byref(res), None),
                 "dp_optimize_sequence": lambda: lib.dp_optimize_sequence(ctx, 4, p, C.byref(fr), C.byref(params), C.byref(st), None, C.byref(sr), None)}
        for who, call in calls.items():
            assert call() == _lib.DP_ERR_DEVICE, who
            assert lib.dp_last_error(ctx).decode() == who + ": the context has no device image"
        bad = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0, kernel=7)
        assert lib.dp_optimize(ctx, C.byref(batch), C.byref(bad), C.byref(res), None) == _lib.DP_ERR_INVALID
        assert "unknown kernel selector" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        buf = (C.c_float * 4096)()
        p = C.cast(buf, C.c_void_p).value
        batch = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        params = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        sk = _lib.DpSkeletonIn(offsets=p, stride=66)
        assert lib.dp_optimize_skeleton(ctx, C.byref(batch), C.byref(params), C.byref(sk), C.byref(_lib.DpResult()), None) == _lib.DP_ERR_UNSUPPORTED
        assert lib.dp_forward_skeleton(ctx, 4, p, p, C.byref(sk), C.byref(_lib.DpResult()), None) == _lib.DP_ERR_UNSUPPORTED
    finally:
        lib.dp_destroy(ctx)


def _model(parents, seed):
    raw = dict(np.load(DEFAULT_MODEL))
    rng = np.random.default_rng(seed)
    if parents is not None:
        raw["parents"] = np.asarray(parents, np.int32)
    off = rng.uniform(-0.25, 0.25, (NJ, 3)).astype(np.float32)
    off[0] = rng.uniform(-1, 1, 3)  # (row 0 is never read: a value there must not show up anywhere)
    raw["offsets"] = off
    return HostModel(DEFAULT_MODEL, arrays=raw), off


@pytest.mark.parametrize("tree", ["xsens"] + list(TREES))
@pytest.mark.parametrize("bp", [0, 1])
def test_the_kernels_row_rule_rebuilds_the_hosts_bone_tables(tree, bp):
    """dp_w4_impl.h (W4_SKEL): side s of quad b reads row bone_slot[s] of its frame's skeleton when it is below 22 and carries zero otherwise;
    quads 0..2 write row init_id of item b as the root child's bone when it is below 22.  That has to be what pairs_w4 / dp_debug_items
    build from the context's own offsets, for every tree the tests use -- and together the rows read must be every bone 1..21, which is
    what lets the kernel screen a frame's skeleton lane by lane."""
    lib = _lib.load()
    hm, off = _model(None if tree == "xsens" else TREES[tree], seed=len(tree) + bp)
    pairs, items = np.zeros(16, PAIR), np.zeros(32, ITEM)
    fn = lib.dp_debug_pairs_w4_bp if bp else lib.dp_debug_pairs_w4
    assert fn(C.byref(hm.struct), pairs.ctypes.data_as(C.c_void_p)) == 0
    assert lib.dp_debug_items(C.byref(hm.struct), items.ctypes.data_as(C.c_void_p)) == 0
    read = set()
    for b in range(16):
        for s in range(2):
            slot = int(pairs["bone_slot"][b, s])
            want = off[slot] if slot < NJ else np.zeros(3, np.float32)
            np.testing.assert_array_equal(pairs["off"][b, :, s], want, err_msg=f"quad {b} side {s}")
            if slot < NJ:
                assert slot >= 1
                read.add(slot)
            else:
                assert slot >= SLOT_TRASH
    for b in range(MAX_ROOT_CH):
        iid = int(items["init_id"][b])
        want = off[iid] if iid < NJ else np.zeros(3, np.float32)
        np.testing.assert_array_equal(items["init_off"][b], want, err_msg=f"root child {b}")
        if iid < NJ:
            read.add(iid)
    assert read == set(range(1, NJ))


def _skel_kernels(tmp_path):
    lib = tmp_path / "libdragposer_hip.so"
    shutil.copy(os.path.join(ROOT, "dragposer_amd", "lib", "libdragposer_hip.so"), lib)
    tool = lambda n: os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", n)
    if not os.path.exists(tool("llvm-objdump")):
        pytest.skip("needs the ROCm LLVM tools")
    subprocess.check_call([tool("llvm-objdump"), "--offloading", lib.name], cwd=tmp_path, stdout=subprocess.DEVNULL)
    found = set()
    for co in (p for p in tmp_path.iterdir() if p.name.startswith(lib.name + ".") and p.name.endswith("gfx950")):
        found |= set(re.findall(r"\b(_Z\d+dp_w4sk(?:_bp)?_kernel\w*)", subprocess.check_output([tool("llvm-readelf"), "-s", "--wide", str(co)], text=True)))
    return found


def test_every_compiled_skeleton_kernel_has_a_gpu_row_and_every_row_exists(tmp_path):
    table = [skel_symbol(i) for i in SKEL_INSTANTIATIONS]
    assert len(set(table)) == len(table) == 12
    assert _skel_kernels(tmp_path) == set(table)
    assert not any(re.match(r"_Z\d+dp_w(?:4|4_bp|16)_kernel\w*", s) for s in table)  # (outside tests/instantiations.py's pattern)


@pytest.mark.parametrize("unit,plain", [("dp_w4_skel.hip", "dp_w4.hip"), ("dp_w4_bp_skel.hip", "dp_w4_bp.hip")])
def test_skeleton_units_keep_the_plain_units_register_budget(unit, plain, tmp_path):
    notes, base = _kernel_notes(unit, tmp_path), _kernel_notes(plain, tmp_path)
    name = "dp_w4sk_bp_kernel" if "bp" in unit else "dp_w4sk_kernel"
    pname = "dp_w4_bp_kernel" if "bp" in plain else "dp_w4_kernel"
    kernels = {k: v for k, v in notes.items() if name in k}
    assert len(kernels) == 6, list(notes)
    lds_plain = max(v["lds"] for k, v in base.items() if pname in k)
    for k, n in kernels.items():
        p = base[k.replace(f"{len(name)}{name}", f"{len(pname)}{pname}")]
        assert n["lds"] <= lds_plain, (k, n)
        if "ILi4ELb1ELb1ELb" in k:  # whole-sequence instantiations: no more than the same instantiation of the plain unit
            assert n["vspill"] <= p["vspill"] and n["scratch"] <= p["scratch"], (k, n, p)
            continue
        # (the accumulator half as the plain unit fills it: all 256 in the dense unit; the body-part one's layer 2 holds 40 registers fewer)
        assert n["vspill"] == 0 and n["scratch"] == 0 and n["agpr"] == p["agpr"], (k, n, p)
        assert "bp" in unit or n["agpr"] == 256, (k, n)


def test_python_shape_and_kernel_errors():
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.optimizer import LatentOptimizer

    fake = types.SimpleNamespace(device=torch.device("cpu"))
    sk = LatentOptimizer._skeleton(fake, torch.zeros(22, 3), 8, "optimize")
    assert sk.stride == 0 and sk.offsets
    assert LatentOptimizer._skeleton(fake, torch.zeros(8, 22, 3), 8, "optimize").stride == 66
    for bad in (torch.zeros(66), torch.zeros(7, 22, 3), torch.zeros(8, 21, 3), torch.zeros(1, 8, 22, 3)):
        with pytest.raises(ValueError):
            LatentOptimizer._skeleton(fake, bad, 8, "optimize")
    with pytest.raises(ValueError):
        LatentOptimizer._skeleton(fake, torch.zeros(8, 22, 3, dtype=torch.float64), 8, "optimize")
    with pytest.raises(ValueError):
        LatentOptimizer._skeleton(fake, torch.zeros(8, 3, 22).transpose(1, 2), 8, "optimize")  # (not contiguous)
    with pytest.raises(TypeError):
        LatentOptimizer._skeleton(fake, np.zeros((22, 3), np.float32), 8, "optimize")
    z = torch.zeros(8, 24)
    with pytest.raises(ValueError, match="w16"):
        LatentOptimizer.plan(fake, z, z, None, None, None, None, None, kernel="w16", offsets=torch.zeros(22, 3))
    dp = types.SimpleNamespace(S=2, device=torch.device("cpu"), offsets=torch.arange(66, dtype=torch.float32).reshape(22, 3),
                               _skel_obj=None, _skel_dev=None)
    for bad in (np.zeros((3, 22, 3)), np.zeros((22, 2)), np.zeros(66)):
        with pytest.raises(ValueError, match="offsets"):
            DragPose._skeleton(dp, bad)
    own = dp.offsets.clone()
    own[0] = 5.0  # (row 0 is ignored)
    assert DragPose._skeleton(dp, own) is None
    assert DragPose._skeleton(dp, own.expand(2, 22, 3).numpy()) is None
    other = own * 1.1
    got = DragPose._skeleton(dp, other)
    assert torch.equal(got, other) and got is not other
    assert DragPose._skeleton(dp, other) is got  # (decided once per object)
