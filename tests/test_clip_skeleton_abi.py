"""CPU: per-sequence skeletons in the joint clip solve and the LM solver (include/dragposer_clip_skeleton.h) -- the header against the C
compiler and the binding, the two calls' refusals on a context without a device in the header's order (the plain calls' own, dp_skeleton_in's,
the workspace), the test-only library's refusal, the two new kernels' register and LDS budget, and what LatentOptimizer refuses before it
reaches the library.  No compute call is made here (the GPU side is tests/test_hip_clip_skeleton.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import __graft_entry__ as G
from dragposer_amd import ClipLM, Terms, _lib
from dragposer_amd.optimizer import LatentOptimizer
from test_build_quality import _kernel_notes
from test_host_san import ROOT
from test_sequence_constraints_abi import _host_ctx

HDR = os.path.join(ROOT, "include", "dragposer_clip_skeleton.h")
SK_LDS = 122576  # dp_lm_skel.h: SK_LDS_BYTES = dp_lm.h's 121 488 + 4 waves x 68 floats


def test_header_declares_the_calls_and_the_library_exports_them():
    text = open(HDR).read()
    assert re.findall(r"^(?:int|size_t)\s+(dp_\w+)\s*\(", text, flags=re.M) == list(_lib.CLIP_SKELETON_SYMBOLS) == ["dp_optimize_clip_lm_skeleton", "dp_optimize_lm_skeleton"]
    assert _lib.CLIP_LM_SYMBOLS == ("dp_clip_lm_workspace_bytes", "dp_optimize_clip_lm")  # (the neighbours' tuples stay)
    lib = _lib.load()
    for sym in _lib.CLIP_SKELETON_SYMBOLS:
        assert hasattr(lib, sym)
    assert "dp_clip_skel.hip" in G.HIP_SOURCES and "dp_lm_skel.hip" in G.HIP_SOURCES
    lds = re.search(r"static_assert\(SK_LDS_BYTES == (\d+)", open(os.path.join(G.CSRC, "dp_lm_skel.h")).read())
    assert int(lds.group(1)) == SK_LDS
    not_covered = text[text.index("Not covered"):text.index("#ifndef")]
    for word in ("dp_optimize_sequence_lm", "dp_optimize_lm_terms", "dp_optimize_sequence_lm_terms", "a skeleton per frame inside one", "DragPose", "plug-in"):
        assert word in not_covered, word
    for word in ("stride 66", "stride 0", "Row 0", "DP_CLIP_REFUSED_FRAME", "DP_STATUS_BAD_STATE", "Refusals", "captured graph", "lambda_accel = 0"):
        assert word in text, word
    assert lib.dp_version() == 510  # (the header is an addition: DP_VERSION stays)


def test_the_header_compiles_as_c_and_as_cxx(tmp_path):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no gcc / g++")
    body = '#include "dragposer_clip_skeleton.h"\nint main(void) { dp_skeleton_in s = {(unsigned)sizeof(dp_skeleton_in), 0u, (const float*)0, 0}; dp_clip_accel_params a = DP_CLIP_ACCEL_PARAMS_INIT; ' \
           'dp_clip_lm_params p = DP_CLIP_LM_PARAMS_INIT; dp_lm_params q = DP_LM_PARAMS_INIT; ' \
           'return (int)(p.n_steps - 4 + q.n_steps - 3 + s.stride + (a.accel_loss != 0)); }\n'
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        src = tmp_path / f"hdr.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _caller(lib):
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    batch = _lib.DpBatch(n_frames=6, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    out = _lib.DpResult(z=p)

    def ext(S=2, B=6, short=0, accel=True, **k):
        s = _lib.DpClipLmExtra(mu=p, n_accepted=p, clip_loss=p, loss_hist=p, info=p, workspace=p)
        s.workspace_bytes = max((lib.dp_clip_lm_accel_workspace_bytes if accel else lib.dp_clip_lm_workspace_bytes)(S, B) - short, 0)
        for key, v in k.items():
            setattr(s, key, v)
        return s

    def acc(**k):
        s = _lib.DpClipAccelParams(lambda_accel=5.0, accel_loss=p)
        for key, v in k.items():
            setattr(s, key, v)
        return s

    def skel(**k):
        s = _lib.DpSkeletonIn()
        s.offsets, s.stride = p, 66
        for key, v in k.items():
            setattr(s, key, v)
        return s

    def clip(ctx, params=None, accel=None, sk=None, extra=None, result=None, b=batch, S=2, null=()):
        prm = params if params is not None else _lib.DpClipLmParams()
        ac = accel if accel is not None else acc()
        ex = extra if extra is not None else ext(S if S > 0 else 2, b.n_frames if b.n_frames > 0 else 6, accel="accel" not in null)
        rs = result if result is not None else out
        s = sk if sk is not None else skel()
        rc = lib.dp_optimize_clip_lm_skeleton(ctx, None if "batch" in null else C.byref(b), S, None if "params" in null else C.byref(prm),
                                              None if "accel" in null else C.byref(ac), None if "skel" in null else C.byref(s), C.byref(rs),
                                              None if "extra" in null else C.byref(ex), None)
        return rc, (lib.dp_last_error(ctx).decode() if ctx else "")

    def lm(ctx, params=None, sk=None, extra=None, result=None, b=batch, null=()):
        prm = params if params is not None else _lib.DpLmParams()
        s = sk if sk is not None else skel()
        rs = result if result is not None else out
        rc = lib.dp_optimize_lm_skeleton(ctx, None if "batch" in null else C.byref(b), None if "params" in null else C.byref(prm),
                                         None if "skel" in null else C.byref(s), C.byref(rs), C.byref(extra) if extra is not None else None, None)
        return rc, (lib.dp_last_error(ctx).decode() if ctx else "")

    return clip, lm, ext, acc, skel, p, buf


def _set(cls, **k):
    s = cls()
    for key, v in k.items():
        setattr(s, key, v)
    return s


def test_clip_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    clip, _, ext, acc, skel, p, buf = _caller(lib)
    nan = float("nan")
    assert clip(None)[0] == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        prm = lambda **k: _set(_lib.DpClipLmParams, **k)
        small = _lib.DpResult(z=p)
        small.struct_size = 8
        bad_batch = _lib.DpBatch(n_frames=0, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        # each stage names what it refuses, with a later stage's fault present as well: the plain calls' own first, in their order ...
        stages = [(dict(null=("batch", "skel")), "NULL batch, params or extra"),
                  (dict(params=prm(struct_size=36), null=("skel",)), "dp_clip_lm_params.struct_size is 36"),
                  (dict(result=small, sk=skel(struct_size=4)), "dp_result.struct_size"),
                  (dict(extra=ext(reserved0=1), sk=skel(reserved0=1)), "dp_clip_lm_extra"),
                  (dict(params=prm(n_steps=0), null=("skel",)), "n_steps 0 outside 1..64"),
                  (dict(params=prm(mu0=5e6), sk=skel(stride=5)), "mu0 outside [mu_min, mu_max]"),
                  (dict(b=bad_batch, null=("skel",)), "n_frames must be positive"),
                  (dict(S=4, null=("skel",)), "n_sequences 4 must be positive and divide n_frames 6"),
                  (dict(params=prm(lambda_smooth=nan), null=("skel",)), "lambda_smooth is negative or not finite"),
                  (dict(accel=acc(struct_size=8), null=("skel",)), "dp_clip_accel_params.struct_size is 8"),
                  (dict(accel=acc(lambda_accel=nan), sk=skel(offsets=None)), "lambda_accel is negative or not finite"),
                  # ... then dp_skeleton_in's, as dp_optimize_skeleton states them ...
                  (dict(null=("skel",), extra=ext(workspace=None)), "the skeleton is NULL"),
                  (dict(null=("skel", "accel"), extra=ext(short=1, accel=False)), "the skeleton is NULL"),
                  (dict(sk=skel(struct_size=8, reserved0=1), extra=ext(workspace=None)), "dp_skeleton_in.struct_size is 8"),
                  (dict(sk=skel(reserved0=1, offsets=None)), "reserved0 1"),
                  (dict(sk=skel(offsets=None, stride=5)), "dp_skeleton_in.offsets is NULL"),
                  (dict(sk=skel(stride=5), extra=ext(workspace=None)), "dp_skeleton_in.stride is 5"),
                  (dict(sk=skel(stride=22), extra=ext(short=1)), "dp_skeleton_in.stride is 22"),
                  # ... then the workspace, against the size function of the form chosen
                  (dict(extra=ext(workspace=None)), "workspace is NULL"),
                  (dict(extra=ext(short=1)), f"fewer than the {lib.dp_clip_lm_accel_workspace_bytes(2, 6)} of dp_clip_lm_accel_workspace_bytes(2, 6)"),
                  (dict(extra=ext(accel=False)), "of dp_clip_lm_accel_workspace_bytes(2, 6)"),  # (dp_optimize_clip_lm's size does not do with `accel` given)
                  (dict(accel=acc(lambda_accel=0.0), extra=ext(short=1)), "fewer than the"),
                  (dict(null=("accel",), extra=ext(short=1, accel=False)), f"fewer than the {lib.dp_clip_lm_workspace_bytes(2, 6)} of dp_clip_lm_workspace_bytes(2, 6)")]
        for kw, word in stages:
            rc, msg = clip(ctx, **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and "dp_optimize_clip_lm_skeleton" in msg, (word, msg)
        # well-formed, both forms and both strides: refused only because there is no device
        for kw in (dict(), dict(null=("accel",)), dict(sk=skel(stride=0)), dict(null=("accel",), sk=skel(stride=0)), dict(S=1), dict(S=6),
                   dict(accel=acc(lambda_accel=0.0)), dict(null=("accel",), extra=ext())):  # (the larger workspace does for the NULL form)
            rc, msg = clip(ctx, **kw)
            assert rc == _lib.DP_ERR_DEVICE and "dp_optimize_clip_lm_skeleton" in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_lm_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    _, lm, _, _, skel, p, buf = _caller(lib)
    assert lm(None)[0] == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        prm = lambda **k: _set(_lib.DpLmParams, **k)
        small = _lib.DpResult(z=p)
        small.struct_size = 8
        null_batch = _lib.DpBatch(n_frames=6, z0=p, z_tgt=None, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        stages = [(dict(null=("params", "skel")), "NULL batch or params"),
                  (dict(params=prm(struct_size=8), null=("skel",)), "dp_lm_params.struct_size is 8"),
                  (dict(result=small, null=("skel",)), "dp_result.struct_size"),
                  (dict(extra=_set(_lib.DpLmExtra, reserved0=1), sk=skel(reserved0=1)), "dp_lm_extra"),
                  (dict(params=prm(n_steps=65), null=("skel",)), "n_steps 65 outside 1..64"),
                  (dict(params=prm(mu_up=1.0), sk=skel(stride=5)), "mu_up must be greater than 1"),
                  (dict(b=null_batch, null=("skel",)), "NULL input array"),
                  (dict(null=("skel",)), "the skeleton is NULL"),
                  (dict(sk=skel(struct_size=8, reserved0=1)), "dp_skeleton_in.struct_size is 8"),
                  (dict(sk=skel(reserved0=1, offsets=None)), "reserved0 1"),
                  (dict(sk=skel(offsets=None, stride=5)), "dp_skeleton_in.offsets is NULL"),
                  (dict(sk=skel(stride=5)), "dp_skeleton_in.stride is 5")]
        for kw, word in stages:
            rc, msg = lm(ctx, **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and "dp_optimize_lm_skeleton" in msg, (word, msg)
        for kw in (dict(), dict(sk=skel(stride=0)), dict(extra=_lib.DpLmExtra(mu=p, n_accepted=p, loss0=p))):
            rc, msg = lm(ctx, **kw)
            assert rc == _lib.DP_ERR_DEVICE and "dp_optimize_lm_skeleton" in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    for sym in _lib.CLIP_SKELETON_SYMBOLS + _lib.CLIP_ACCEL_SYMBOLS + _lib.CLIP_LM_SYMBOLS:
        getattr(lib, sym).argtypes, getattr(lib, sym).restype = getattr(_lib.load(), sym).argtypes, getattr(_lib.load(), sym).restype
    clip, lm, ext, acc, skel, p, buf = _caller(lib)
    ctx = _host_ctx(lib)
    try:
        for call in (clip, lm):
            rc, msg = call(ctx)
            assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in msg
            assert call(ctx, sk=skel(stride=7))[0] == _lib.DP_ERR_INVALID  # (its argument checks come first)
    finally:
        lib.dp_destroy(ctx)
    del buf


@pytest.mark.parametrize("src,kernel,vgpr", [("dp_clip_skel.hip", "dp_clip_rows_skel_kernel", 128), ("dp_lm_skel.hip", "dp_lm_skel_kernel", 400)])  # (128 and 392)
def test_the_kernels_keep_their_budget(tmp_path, src, kernel, vgpr):
    """hipcc -S with the build's flags: no spilled vector register, no scratch, and the LDS figure the header states -- dp_lm.h's array and a
    68-float block of bones per wave, one workgroup per CU"""
    notes = _kernel_notes(src, tmp_path)
    assert len(notes) == 1
    (name, n), = notes.items()
    assert kernel in name
    assert n["vspill"] == 0 and n["scratch"] == 0, n
    assert n["lds"] == SK_LDS <= 160 * 1024 and n["vgpr"] <= vgpr, n
    assert not re.search(r"dp_w4\w*_kernel|dp_w16_kernel", name)  # (tests/test_instantiation_coverage.py claims these patterns)


def _bare_optimizer():
    opt = LatentOptimizer.__new__(LatentOptimizer)
    opt.device, opt.lib = torch.device("cpu"), None  # (every refusal below comes before the library is reached)
    opt.ctx = C.c_void_p()
    return opt


def test_python_refuses_shapes_and_terms_without_a_library():
    opt = _bare_optimizer()
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    B, S = 6, 2
    frame = dict(z0=z(B, 24), z_tgt=z(B, 24), cur_rot=z(B, 4), tgt_pos=z(B, 22, 3), tgt_rot=z(B, 22, 9), w=z(B, 22, 2), tracked=z(B, 22, dtype=torch.uint8))
    with pytest.raises(ValueError, match="offsets does not go with terms"):
        LatentOptimizer.optimize_lm(opt, **frame, terms=Terms([]), offsets=z(22, 3))
    for bad in (z(66), z(1, 1, 22, 3)):
        with pytest.raises(ValueError, match=r"optimize_lm: offsets must be \[22,3\] \(one skeleton\) or \[6,22,3\]"):
            LatentOptimizer.optimize_lm(opt, **frame, offsets=bad)
        with pytest.raises(ValueError, match=r"optimize_clip_lm: offsets must be \[22,3\] \(one skeleton\) or \[2,22,3\]"):
            LatentOptimizer.optimize_clip_lm(opt, **frame, n_sequences=S, offsets=bad)
    with pytest.raises(ValueError, match=r"offsets: expected contiguous torch.float32 of shape \(6, 22, 3\)"):  # one skeleton per FRAME in optimize_lm ...
        LatentOptimizer.optimize_lm(opt, **frame, offsets=z(S, 22, 3))
    with pytest.raises(ValueError, match=r"offsets: expected contiguous torch.float32 of shape \(2, 22, 3\)"):  # ... and one per SEQUENCE in optimize_clip_lm
        LatentOptimizer.optimize_clip_lm(opt, **frame, n_sequences=S, offsets=z(B, 22, 3))
    with pytest.raises(ValueError, match=r"offsets: expected contiguous torch.float32 of shape \(22, 3\)"):
        LatentOptimizer.optimize_clip_lm(opt, **frame, n_sequences=S, offsets=z(22, 4))
    with pytest.raises(ValueError, match="offsets: expected contiguous torch.float32"):
        LatentOptimizer.optimize_clip_lm(opt, **frame, n_sequences=S, offsets=z(S, 22, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match="offsets must be a torch.Tensor"):
        LatentOptimizer.optimize_clip_lm(opt, **frame, n_sequences=S, clip=ClipLM(accel=5.0), offsets=[[0.0] * 3] * 22)
    with pytest.raises(ValueError, match="n_sequences 4 must be positive"):  # (the plain call's own refusal first)
        LatentOptimizer.optimize_clip_lm(opt, **frame, n_sequences=4, offsets=z(5))
