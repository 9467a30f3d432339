"""CPU: dp_optimize_sequence_constrained and dp_optimize_sequence_terms (include/dragposer_sequence_constraints.h), whole-sequence launches
with the reference's extra loss terms or a term table -- header, binding, exports, the order of the argument refusals on a context without
a device, the test-only library's refusal, and the kernels' register and LDS budget.  No compute call is made here (the GPU side is
tests/test_hip_sequence_constraints.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)
from test_terms_abi import _good_terms, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_sequence_constraints.h")
NAMES = ("dp_optimize_sequence_constrained", "dp_optimize_sequence_terms")
EXTRA_FIELDS = ("struct_size", "reserved0", "loss_extra", "loss_terms", "joint_pos", "row_step")
SQ_LDS = (73008, 76464)  # dp_cons_seq.h: SQ_LDS_BYTES, SQ_LDS_BYTES_T (dp_cons_skel.h's layout: the carried state lives in registers)


def test_header_declares_both_calls_and_the_library_exports_them():
    text = open(HDR).read()
    assert set(re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M)) == set(NAMES) == set(_lib.SEQUENCE_CONSTRAINT_SYMBOLS)
    lib = _lib.load()
    for sym in NAMES:
        assert hasattr(lib, sym), sym
    assert "dp_cons_seq.hip" in G.HIP_SOURCES


def test_seq_extra_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "seq.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_sequence_constraints.h"\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(dp_seq_extra));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_seq_extra, {f}));\n' for f in EXTRA_FIELDS)
                   + 'dp_seq_extra e = DP_SEQ_EXTRA_INIT;\nint any = 0;\nfor (int k = 0; k < DP_MAX_TERMS; ++k) any |= e.row_step[k];\n'
                   'printf("%u %u %d %d %d %d %zu\\n", e.struct_size, e.reserved0, e.loss_extra != 0, e.loss_terms != 0, e.joint_pos != 0, any,'
                   ' sizeof(e.row_step) / sizeof(e.row_step[0]));\nreturn 0; }\n')
    exe = tmp_path / "seq"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert int(lines[0]) == C.sizeof(_lib.DpSeqExtra)
    assert [int(x) for x in lines[1:1 + len(EXTRA_FIELDS)]] == [getattr(_lib.DpSeqExtra, f).offset for f in EXTRA_FIELDS]
    e = _lib.DpSeqExtra()
    assert [int(x) for x in lines[-1].split()] == [e.struct_size, 0, 0, 0, 0, 0, _lib.DP_MAX_TERMS] and not any(e.row_step)


def _args():
    """well-formed arguments of both calls over one host buffer (never dereferenced: no launch is reached)"""
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    fr = _lib.DpSeqFrames(n_steps=3, tgt_pos=p, tgt_rot=p, tgt_root=None, w=p, tracked=p, z_tgt=p, z_tgt_step=0, z_tgt_seq=24)
    prm = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
    st = _lib.DpSeqState(global_pos=p, global_rot=p, latent_buf=p, disp_buf=p, heights_buf=p, history=60, n_heights=2)
    st.height_joints[0], st.height_joints[1] = 4, 8
    adj = _lib.DpSeqStep(adjust_joint=0, adjust_target_joint=4, adjust_weight=0.5)
    res = _lib.DpSeqResults(hist_scratch=p)
    return buf, p, fr, prm, st, adj, res


def _own(which, p):
    if which == 0:
        return _lib.DpConstraints(w_feet_floor=1.0, w_head_hips_forward=2.0), None
    arr = _table(_good_terms())
    return _lib.DpTerms(n_terms=5, terms=C.cast(arr, C.c_void_p)), arr


def _host_ctx(lib):
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK and ctx.value  # a context with no device behind it
    return ctx


@pytest.mark.parametrize("which", (0, 1))
def test_refusals_come_in_the_documented_order_before_any_device_is_touched(which):
    lib = _lib.load()
    fn = getattr(lib, NAMES[which])
    buf, p, fr, prm, st, adj, res = _args()
    own, keep = _own(which, p)
    strct = ("dp_constraints", "dp_terms")[which]
    assert fn(None, 4, p, C.byref(fr), C.byref(prm), C.byref(own), None, C.byref(st), C.byref(adj), C.byref(res), None, None) == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        def call(n=4, latent=p, frames=C.byref(fr), params=C.byref(prm), ext=C.byref(own), sk=None, state=C.byref(st), step=C.byref(adj),
                 out=C.byref(res), extra=None):
            rc = fn(ctx, n, latent, frames, params, ext, sk, state, step, out, extra, None)
            return rc, lib.dp_last_error(ctx).decode()

        for kw in (dict(n=0), dict(latent=None), dict(frames=None), dict(params=None), dict(ext=None), dict(state=None), dict(out=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg and NAMES[which] in msg, kw
        # one bad argument of every stage; each names its struct
        bad_prm = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        bad_prm.struct_size = 8
        bad_res = _lib.DpSeqResults(hist_scratch=p)
        bad_res.reserved0 = 7
        bad_own = type(own)()
        bad_own.struct_size = 8
        bad_extra = _lib.DpSeqExtra()
        bad_extra.struct_size = 12
        bad_sk = _lib.DpSkeletonIn(offsets=p.value, stride=5)
        bad_fr = _lib.DpSeqFrames(n_steps=0, tgt_pos=p, tgt_rot=p, w=p, tracked=p, z_tgt=p, z_tgt_seq=24)
        bad_adam = _lib.DpParams(n_iter=10, lr=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        stages = [(dict(params=C.byref(bad_prm)), "dp_params.struct_size"), (dict(out=C.byref(bad_res)), "dp_seq_results.struct_size"),
                  (dict(ext=C.byref(bad_own)), strct + ".struct_size"), (dict(extra=C.byref(bad_extra)), "dp_seq_extra.struct_size"),
                  (dict(sk=C.byref(bad_sk)), "dp_skeleton_in.stride"), (dict(frames=C.byref(bad_fr)), "n_steps must be positive"),
                  (dict(params=C.byref(bad_adam)), "Adam")]
        for i, (kw, word) in enumerate(stages):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and NAMES[which] in msg, (kw, msg)
            # ... and is reported before every later stage's fault (bad_adam is well-formed up to Adam: it stands in for `params` there)
            later = {}
            for kw2, _ in stages[i + 1:]:
                later.update(kw2)
            if "params" in kw:
                later.pop("params", None)
            rc, msg = call(**{**later, **kw})
            assert rc == _lib.DP_ERR_INVALID and word in msg, (i, msg)
        # the rest of each struct's own rules
        e = _lib.DpSeqExtra()
        e.row_step[3] = -4
        rc, msg = call(extra=C.byref(e))
        assert rc == _lib.DP_ERR_INVALID and "row_step[3]" in msg
        e = _lib.DpSeqExtra()
        e.reserved0 = 1
        assert call(extra=C.byref(e))[0] == _lib.DP_ERR_INVALID
        other = (C.c_float * 16)()
        for field, word in (("global_pos", "global_pos must be NULL or dp_seq_state.global_pos"),
                            (("loss_extra", "loss_terms")[which], "dp_seq_extra." + ("loss_extra", "loss_terms")[which])):
            o2, k2 = _own(which, p)
            setattr(o2, field, C.cast(other, C.c_void_p))
            rc, msg = call(ext=C.byref(o2))
            assert rc == _lib.DP_ERR_INVALID and word in msg and strct in msg, msg
        o2, k2 = _own(which, p)
        o2.global_pos = p  # the state's own array: accepted
        assert call(ext=C.byref(o2))[0] == _lib.DP_ERR_DEVICE
        rc, msg = call(sk=C.byref(_lib.DpSkeletonIn(stride=66)))
        assert rc == _lib.DP_ERR_INVALID and "offsets is NULL" in msg
        bad_st = _lib.DpSeqState(global_pos=p, global_rot=p, latent_buf=p, disp_buf=p, heights_buf=p, history=60, n_heights=9)
        rc, msg = call(state=C.byref(bad_st))
        assert rc == _lib.DP_ERR_INVALID and "n_heights" in msg
        bad_st = _lib.DpSeqState(global_pos=p, global_rot=p, latent_buf=p, disp_buf=p, heights_buf=p, history=60, n_heights=1)
        bad_st.height_joints[0] = 22
        assert call(state=C.byref(bad_st))[0] == _lib.DP_ERR_INVALID
        rc, msg = call(step=C.byref(_lib.DpSeqStep(adjust_joint=3, adjust_target_joint=22)))
        assert rc == _lib.DP_ERR_INVALID and "joint adjustment" in msg
        rc, msg = call(out=C.byref(_lib.DpSeqResults()))
        assert rc == _lib.DP_ERR_INVALID and "hist_scratch" in msg
        # well-formed, with and without a skeleton, extra and joint adjustment: refused only because there is no device
        for kw in (dict(), dict(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=66))), dict(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=0))),
                   dict(extra=C.byref(_lib.DpSeqExtra())), dict(step=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_DEVICE and NAMES[which] in msg, (kw, rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del keep, buf


@pytest.mark.parametrize("which", (0, 1))
def test_the_test_only_library_declines(which):
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        buf, p, fr, prm, st, adj, res = _args()
        own, keep = _own(which, p)
        fn = getattr(lib, NAMES[which])
        rc = fn(ctx, 4, p, C.byref(fr), C.byref(prm), C.byref(own), None, C.byref(st), C.byref(adj), C.byref(res), None, None)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)


def test_sequence_kernels_keep_the_budget(tmp_path):
    notes = _kernel_notes("dp_cons_seq.hip", tmp_path)
    assert len(notes) == 2, list(notes)
    (nc, c), = [(k, v) for k, v in notes.items() if "dp_cons_seq_kernel" in k]
    (nt, t), = [(k, v) for k, v in notes.items() if "dp_terms_seq_kernel" in k]
    assert (c["lds"], t["lds"]) == SQ_LDS
    for name, n in ((nc, c), (nt, t)):
        assert n["vspill"] == 0 and n["scratch"] == 0, (name, n)
        # the unified register file: 512 per SIMD lane, so at most 256 for two waves per SIMD, as the per-frame kernels
        assert n["vgpr"] + n["agpr"] <= 256, (name, n)
        assert not re.search(r"dp_w(4|4_bp|16)_kernel", name)  # (tests/test_instantiation_coverage.py counts those)


def test_python_refuses_what_cannot_be_a_sequence_launch():
    import types

    import torch

    from dragposer_amd import Constraints, Terms
    from dragposer_amd.optimizer import LatentOptimizer

    fake = types.SimpleNamespace(device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    T, S = 3, 2
    a = (torch.zeros(S, 24), torch.zeros(T, S, 22, 3), torch.zeros(T, S, 22, 9), None, torch.zeros(S, 22, 2), torch.zeros(S, 22, dtype=torch.uint8),
         torch.zeros(S, 24), (0, 24), torch.zeros(S, 3), torch.zeros(S, 4), torch.zeros(S, 60, 24), torch.zeros(S, 60, 3), torch.zeros(S, 60, 2), (4, 8))
    with pytest.raises(ValueError, match="not both"):
        LatentOptimizer.optimize_sequence(fake, *a, constraints=Constraints.reference(), terms=Terms())
    with pytest.raises(ValueError, match="outputs of"):
        LatentOptimizer.optimize_sequence(fake, *a, loss_extra=torch.zeros(T, S, 4))
    from dragposer_amd.terms import Term

    for bad in (torch.zeros(T + 1, S, 4), torch.zeros(S + 1, 4), torch.zeros(T, S, 3)):
        with pytest.raises(ValueError, match="per_frame"):
            Terms([Term.plane(4, (0.0, 1.0, 0.0), per_frame=bad)]).to_struct(S, torch.device("cpu"), steps=T)
    ts = Terms([Term.plane(4, (0.0, 1.0, 0.0), per_frame=torch.zeros(T, S, 4)), Term.plane(8, (0.0, 1.0, 0.0), per_frame=torch.zeros(S, 4)),
                Term.distance(3, 7, hi=0.2)])
    assert ts.row_steps(S) == [4 * S, 0, 0]
    cut = ts.frames(1, 3)
    assert tuple(cut.terms[0].per_frame.shape) == (2, S, 4) and cut.terms[0].per_frame.data_ptr() == ts.terms[0].per_frame[1:].data_ptr()
    assert cut.terms[1].per_frame is ts.terms[1].per_frame and cut.terms[2] is ts.terms[2]
