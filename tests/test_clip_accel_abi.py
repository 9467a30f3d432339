"""CPU: the joint clip call with the acceleration term (include/dragposer_clip_accel.h) -- the header against the C compiler and the binding,
the refusals of dp_optimize_clip_lm_accel on a context without a device in the header's order, dp_clip_lm_accel_workspace_bytes against what
the launch accepts, the test-only library's refusal, what ClipLM(accel=...).check() refuses, and the two kernels' register and LDS budget.
No compute call is made here (the GPU side is tests/test_hip_clip_accel.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import ClipLM, _lib
from test_build_quality import _kernel_notes
from test_host_san import ROOT
from test_sequence_constraints_abi import _host_ctx

HDR = os.path.join(ROOT, "include", "dragposer_clip_accel.h")
FIELDS = ("struct_size", "lambda_accel", "accel_loss")
CHAIN_LDS = 15168  # dp_clip_accel.h: CHAIN_LDS_BYTES


def test_header_declares_the_calls_and_the_library_exports_them():
    text = open(HDR).read()
    assert re.findall(r"^(?:int|size_t)\s+(dp_\w+)\s*\(", text, flags=re.M) == list(_lib.CLIP_ACCEL_SYMBOLS) == ["dp_clip_lm_accel_workspace_bytes", "dp_optimize_clip_lm_accel"]
    lib = _lib.load()
    for sym in _lib.CLIP_ACCEL_SYMBOLS:
        assert hasattr(lib, sym)
    assert "dp_clip.hip" in G.HIP_SOURCES and "dp_clip_accel.hip" in G.HIP_SOURCES
    lds = re.search(r"static_assert\(CHAIN_LDS_BYTES == (\d+)", open(os.path.join(G.CSRC, "dp_clip_accel.h")).read())
    assert int(lds.group(1)) == CHAIN_LDS
    for word in ("Not covered", "term tables", "points", "holds", "gaps", "tethers", "per-frame skeletons", "cyclic-reduction", "DragPose", "plug-in", "Conditioning", "T^4",
                 "Refusals"):
        assert word in text, word
    # the neighbour no longer lists the term among what is missing, and says where it is
    neighbour = open(os.path.join(ROOT, "include", "dragposer_clip_lm.h")).read()
    not_covered = neighbour[neighbour.index("Not covered"):neighbour.index("#ifndef")]
    assert "block-pentadiagonal" not in not_covered and "dragposer_clip_accel.h" in neighbour
    assert lib.dp_version() == 510  # (the header is an addition: DP_VERSION stays)


def test_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "accel.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_clip_accel.h"\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(dp_clip_accel_params));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_clip_accel_params, {f}));\n' for f in FIELDS)
                   + 'dp_clip_accel_params a = DP_CLIP_ACCEL_PARAMS_INIT;\nprintf("%u %.9g %d\\n", a.struct_size, a.lambda_accel, a.accel_loss != 0);\nreturn 0; }\n')
    exe = tmp_path / "accel"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert int(lines[0]) == C.sizeof(_lib.DpClipAccelParams) == 16
    assert [int(x) for x in lines[1:4]] == [getattr(_lib.DpClipAccelParams, f).offset for f in FIELDS] == [0, 4, 8]
    a = _lib.DpClipAccelParams()
    assert lines[4].split() == ["16", "0", "0"] and (a.struct_size, a.lambda_accel, a.accel_loss) == (16, 0.0, None)
    assert ClipLM().accel is None and ClipLM(accel=2.5).accel_struct().lambda_accel == 2.5 and ClipLM(accel=0.0).accel_struct().struct_size == 16


def test_the_header_compiles_as_c_and_as_cxx(tmp_path):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no gcc / g++")
    body = '#include "dragposer_clip_accel.h"\nint main(void) { dp_clip_accel_params a = DP_CLIP_ACCEL_PARAMS_INIT; dp_clip_lm_params p = DP_CLIP_LM_PARAMS_INIT; ' \
           'return (int)(p.n_steps - 4 + (a.accel_loss != 0)); }\n'
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        src = tmp_path / f"hdr.{ext}"
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _caller(lib):
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    batch = _lib.DpBatch(n_frames=6, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    out = _lib.DpResult(z=p)

    def ext(S=2, B=6, short=0, **k):
        s = _lib.DpClipLmExtra(mu=p, n_accepted=p, clip_loss=p, loss_hist=p, info=p, workspace=p)
        s.workspace_bytes = max(lib.dp_clip_lm_accel_workspace_bytes(S, B) - short, 0)
        for key, v in k.items():
            setattr(s, key, v)
        return s

    def acc(**k):
        s = _lib.DpClipAccelParams(lambda_accel=5.0, accel_loss=p)
        for key, v in k.items():
            setattr(s, key, v)
        return s

    def call(ctx, params=None, accel=None, extra=None, result=None, b=batch, S=2, null=()):
        prm = params if params is not None else _lib.DpClipLmParams()
        ac = accel if accel is not None else acc()
        ex = extra if extra is not None else ext(S if S > 0 else 2, b.n_frames if b.n_frames > 0 else 6)
        rs = result if result is not None else out
        rc = lib.dp_optimize_clip_lm_accel(ctx, None if "batch" in null else C.byref(b), S, None if "params" in null else C.byref(prm),
                                           None if "accel" in null else C.byref(ac), C.byref(rs), None if "extra" in null else C.byref(ex), None)
        return rc, (lib.dp_last_error(ctx).decode() if ctx else "")

    return call, ext, acc, p, buf


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    call, ext, acc, p, buf = _caller(lib)
    nan, inf = float("nan"), float("inf")
    assert call(None)[0] == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        for null in ("batch", "params", "extra"):
            rc, msg = call(ctx, null=(null, "accel"))
            assert rc == _lib.DP_ERR_INVALID and "NULL batch, params or extra" in msg, msg

        def prm(**k):
            s = _lib.DpClipLmParams()
            for key, v in k.items():
                setattr(s, key, v)
            return s

        small = _lib.DpResult(z=p)
        small.struct_size = 8
        bad_batch = _lib.DpBatch(n_frames=0, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        null_batch = _lib.DpBatch(n_frames=6, z0=p, z_tgt=None, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        old_size = lib.dp_clip_lm_workspace_bytes(2, 6)
        # each stage names what it refuses, with a later stage's fault present as well: dp_optimize_clip_lm's stages first, in its order
        stages = [(dict(params=prm(struct_size=36, n_steps=0), accel=acc(struct_size=4)), "dp_clip_lm_params.struct_size is 36"),
                  (dict(result=small, params=prm(n_steps=0)), "dp_result.struct_size"),
                  (dict(extra=ext(struct_size=56), params=prm(n_steps=0)), "dp_clip_lm_extra.struct_size is 56"),
                  (dict(extra=ext(reserved0=1), params=prm(n_steps=0)), "reserved0 1"),
                  (dict(params=prm(n_steps=0, lambda_rot=nan)), "n_steps 0 outside 1..64"),
                  (dict(params=prm(lambda_rot=nan, mu_down=2.0)), "lambda_rot or lambda_tmp"),
                  (dict(params=prm(mu0=nan, mu_down=2.0)), "is not finite"),
                  (dict(params=prm(mu_down=1.0, mu_up=1.0)), "mu_down must lie in (0, 1)"),
                  (dict(params=prm(mu_up=1.0, mu_min=2.0, mu_max=1.0)), "mu_up must be greater than 1"),
                  (dict(params=prm(mu_min=2.0, mu_max=1.0, mu0=5.0)), "0 < mu_min <= mu_max"),
                  (dict(params=prm(mu0=5e6), b=bad_batch), "mu0 outside [mu_min, mu_max]"),
                  (dict(b=bad_batch, S=0), "n_frames must be positive"),
                  (dict(b=null_batch, S=0), "NULL input array"),
                  (dict(S=0, params=prm(lambda_smooth=nan)), "n_sequences 0 must be positive and divide n_frames 6"),
                  (dict(S=4, params=prm(lambda_smooth=-1.0)), "n_sequences 4 must be positive and divide n_frames 6"),
                  (dict(params=prm(lambda_smooth=nan), null=("accel",)), "lambda_smooth is negative or not finite"),
                  (dict(params=prm(lambda_smooth=-0.5), accel=acc(struct_size=4)), "lambda_smooth is negative or not finite"),
                  # ... then the new struct, its value, and the workspace against the new size function
                  (dict(null=("accel",), extra=ext(workspace=None)), "dp_clip_accel_params is NULL"),
                  (dict(accel=acc(struct_size=8, lambda_accel=nan)), "dp_clip_accel_params.struct_size is 8"),
                  (dict(accel=acc(struct_size=5000), extra=ext(short=1)), "dp_clip_accel_params.struct_size is 5000"),
                  (dict(accel=acc(lambda_accel=nan), extra=ext(workspace=None)), "lambda_accel is negative or not finite"),
                  (dict(accel=acc(lambda_accel=-0.5), extra=ext(short=1)), "lambda_accel is negative or not finite"),
                  (dict(accel=acc(lambda_accel=inf)), "lambda_accel is negative or not finite"),
                  (dict(extra=ext(workspace=None)), "workspace is NULL"),
                  (dict(extra=ext(short=1)), f"fewer than the {lib.dp_clip_lm_accel_workspace_bytes(2, 6)} of dp_clip_lm_accel_workspace_bytes(2, 6)"),
                  (dict(extra=ext(workspace_bytes=old_size)), "fewer than the"),  # (dp_optimize_clip_lm's size does not do)
                  (dict(accel=acc(lambda_accel=0.0), extra=ext(short=1)), "fewer than the"),  # (nor at lambda_accel 0: one size per entry point)
                  (dict(extra=ext(S=1, B=3), S=3), "fewer than the")]
        for kw, word in stages:
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and "dp_optimize_clip_lm_accel" in msg, (word, msg)
        # well-formed, every optional pointer given or NULL, S = 1 and S = B, lambda_accel 0: refused only because there is no device
        bare = _lib.DpClipLmExtra(workspace=p)
        bare.workspace_bytes = lib.dp_clip_lm_accel_workspace_bytes(2, 6)
        for kw in (dict(), dict(extra=bare, accel=acc(accel_loss=None)), dict(S=1), dict(S=6), dict(S=3), dict(accel=acc(lambda_accel=0.0)),
                   dict(params=prm(n_steps=64, lambda_smooth=0.0)), dict(extra=ext(short=-1000))):
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_DEVICE and "dp_optimize_clip_lm_accel" in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_workspace_bytes_is_monotone_and_zero_for_what_the_call_refuses():
    lib = _lib.load()
    ws, old = lib.dp_clip_lm_accel_workspace_bytes, lib.dp_clip_lm_workspace_bytes
    assert [ws(*a) for a in ((0, 6), (-1, 6), (2, 0), (2, -4), (4, 6), (7, 6))] == [0] * 6
    prev = 0
    for T in (1, 2, 3, 7, 33, 65, 240, 5052):
        for S in (1, 2, 5, 64):
            n = ws(S, S * T)
            assert n > 0 and n % 16 == 0
            # per frame: two latents, A | g, L^-1 | y | F, two loss rows, two first-difference parts, the flags; per sequence: 40 bytes; 16-byte
            # rounding of 14 parts
            per_frame, per_seq = 2 * 96 + 2400 + 4704 + 2 * 16 + 2 * 8 + 4, 16 + 4 * 4 + 8
            assert S * T * per_frame + S * per_seq <= n <= S * T * per_frame + S * per_seq + 14 * 15, (S, T, n)
            assert n >= old(S, S * T) + S * T * 2304
        assert ws(1, T) > prev
        prev = ws(1, T)
    assert ws(3, 6) < ws(3, 9) and ws(2, 6) != 0 and ws(1, 5052) < 2 ** 31
    # the byte counts themselves (n_sequences, n_frames): both calls size one list, dp_clip.h's, and a caller's allocation must keep fitting
    assert [ws(*a) for a in ((1, 1), (3, 9), (2, 130), (1, 5052))] == [7472, 66304, 955360, 37122192]


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    for sym in _lib.CLIP_ACCEL_SYMBOLS + _lib.CLIP_LM_SYMBOLS:
        getattr(lib, sym).argtypes, getattr(lib, sym).restype = getattr(_lib.load(), sym).argtypes, getattr(_lib.load(), sym).restype
    call, ext, acc, p, buf = _caller(lib)
    ctx = _host_ctx(lib)
    try:
        rc, msg = call(ctx)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in msg
        assert call(ctx, accel=acc(lambda_accel=-1.0))[0] == _lib.DP_ERR_INVALID  # (its argument checks come first)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_clip_check_refuses_what_the_library_would():
    ClipLM(accel=0.0).check()
    ClipLM(steps=64, smooth=0.0, accel=500.0).check()
    for bad in (-1.0, float("nan"), float("inf"), -0.0001):
        with pytest.raises(ValueError, match="accel is negative or not finite"):
            ClipLM(accel=bad).check()
    with pytest.raises(ValueError, match="smooth is negative or not finite"):  # (in the library's order: smooth first)
        ClipLM(smooth=-1.0, accel=-1.0).check()
    s = ClipLM(5, smooth=2.5, accel=7.0)
    assert s.to_struct(2.0, 0.5).lambda_smooth == 2.5 and s.accel_struct().lambda_accel == 7.0
    assert C.sizeof(_lib.DpClipLmParams) == 40  # (the neighbour's struct has not grown)


def test_the_kernels_keep_their_budget(tmp_path):
    """hipcc -S with the build's flags: no spilled vector register, no scratch, and the LDS figure the header states"""
    notes = _kernel_notes("dp_clip_accel.hip", tmp_path)
    assert len(notes) == 2
    pick = lambda word: [n for name, n in notes.items() if word in name]
    chain, decide = pick("dp_clip_accel_chain_kernel"), pick("dp_clip_accel_decide_kernel")
    assert len(chain) == len(decide) == 1
    for n in chain + decide:
        assert n["vspill"] == 0 and n["scratch"] == 0, n
    assert chain[0]["lds"] == CHAIN_LDS and chain[0]["vgpr"] <= 512, chain[0]  # (a lone wave per workgroup)
    assert decide[0]["lds"] == 0 and decide[0]["vgpr"] <= 64, decide[0]
    for name in notes:  # tests/test_instantiation_coverage.py claims these patterns for the optimise kernels
        assert not re.search(r"dp_w4\w*_kernel|dp_w16_kernel|dp_lm\w*_kernel", name)
