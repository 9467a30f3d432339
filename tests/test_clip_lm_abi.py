"""CPU: the joint clip call (include/dragposer_clip_lm.h) -- the header against the C compiler and the binding, the refusals of
dp_optimize_clip_lm on a context without a device in the header's order, dp_clip_lm_workspace_bytes against what the launch accepts, the
test-only library's refusal, what ClipLM.check() refuses, and the three kernels' register and LDS budget.  No compute call is made here (the
GPU side is tests/test_hip_clip_lm.py)."""
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

HDR = os.path.join(ROOT, "include", "dragposer_clip_lm.h")
PARAMS_FIELDS = ("struct_size", "n_steps", "lambda_rot", "lambda_tmp", "lambda_smooth", "mu0", "mu_up", "mu_down", "mu_min", "mu_max")
EXTRA_FIELDS = ("struct_size", "reserved0", "mu", "n_accepted", "clip_loss", "loss_hist", "info", "workspace", "workspace_bytes")
ROWS_LDS = 121488  # dp_lm.h: LDS_BYTES, the rows kernel's
CHAIN_LDS = 8480   # dp_clip.h: CHAIN_LDS_BYTES


def test_header_declares_the_calls_and_the_library_exports_them():
    text = open(HDR).read()
    assert re.findall(r"^(?:int|size_t)\s+(dp_\w+)\s*\(", text, flags=re.M) == list(_lib.CLIP_LM_SYMBOLS) == ["dp_clip_lm_workspace_bytes", "dp_optimize_clip_lm"]
    lib = _lib.load()
    for sym in _lib.CLIP_LM_SYMBOLS:
        assert hasattr(lib, sym)
    assert re.search(r"#define DP_CLIP_REFUSED_FRAME 1\b", text) and _lib.DP_CLIP_REFUSED_FRAME == 1
    assert "dp_clip.hip" in G.HIP_SOURCES
    lds = re.search(r"static_assert\(CHAIN_LDS_BYTES == (\d+)", open(os.path.join(G.CSRC, "dp_clip.h")).read())
    assert int(lds.group(1)) == CHAIN_LDS
    for word in ("Not covered", "second-difference", "cyclic-reduction", "plug-in", "per-frame skeletons"):
        assert word in text, word
    assert lib.dp_version() == 510  # (the header is an addition: DP_VERSION stays)


def test_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "clip.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_clip_lm.h"\nint main(void) {\n'
                   'printf("%zu %zu %d\\n", sizeof(dp_clip_lm_params), sizeof(dp_clip_lm_extra), DP_CLIP_REFUSED_FRAME);\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_clip_lm_params, {f}));\n' for f in PARAMS_FIELDS)
                   + "".join(f'printf("%zu\\n", offsetof(dp_clip_lm_extra, {f}));\n' for f in EXTRA_FIELDS)
                   + 'dp_clip_lm_params p = DP_CLIP_LM_PARAMS_INIT;\ndp_clip_lm_extra e = DP_CLIP_LM_EXTRA_INIT;\n'
                   'printf("%u %d\\n", p.struct_size, p.n_steps);\n'
                   'printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\\n", p.lambda_rot, p.lambda_tmp, p.lambda_smooth, p.mu0, p.mu_up, p.mu_down, p.mu_min, p.mu_max);\n'
                   'printf("%u %u %d %d %d %d %d %d %zu\\n", e.struct_size, e.reserved0, e.mu != 0, e.n_accepted != 0, e.clip_loss != 0, e.loss_hist != 0, '
                   'e.info != 0, e.workspace != 0, e.workspace_bytes);\nreturn 0; }\n')
    exe = tmp_path / "clip"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpClipLmParams), C.sizeof(_lib.DpClipLmExtra), _lib.DP_CLIP_REFUSED_FRAME] == [40, 64, 1]
    n = len(PARAMS_FIELDS)
    assert [int(x) for x in lines[1:1 + n]] == [getattr(_lib.DpClipLmParams, f).offset for f in PARAMS_FIELDS] == list(range(0, 40, 4))
    assert [int(x) for x in lines[1 + n:1 + n + len(EXTRA_FIELDS)]] == [getattr(_lib.DpClipLmExtra, f).offset for f in EXTRA_FIELDS] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    p, e, d = _lib.DpClipLmParams(), _lib.DpClipLmExtra(), ClipLM()
    assert [int(x) for x in lines[-3].split()] == [p.struct_size, p.n_steps] == [40, 4] and d.steps == 4
    f32 = lambda x: C.c_float(x).value
    floats = [f32(float(x)) for x in lines[-2].split()]  # (%.9g round-trips a float)
    assert floats == [p.lambda_rot, p.lambda_tmp, p.lambda_smooth, p.mu0, p.mu_up, p.mu_down, p.mu_min, p.mu_max]
    assert floats[2:] == [f32(d.smooth), f32(d.mu0), f32(d.mu_up), f32(d.mu_down), f32(d.mu_min), f32(d.mu_max)] == [1.0, f32(1e-2), 4.0, f32(1.0 / 3.0), f32(1e-6), 1e6]
    assert [int(x) for x in lines[-1].split()] == [e.struct_size, 0, 0, 0, 0, 0, 0, 0, 0]
    assert (e.reserved0, e.mu, e.n_accepted, e.clip_loss, e.loss_hist, e.info, e.workspace, e.workspace_bytes) == (0, None, None, None, None, None, None, 0)


def test_the_header_compiles_as_c_and_as_cxx(tmp_path):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no gcc / g++")
    body = '#include "dragposer_clip_lm.h"\nint main(void) { dp_clip_lm_params p = DP_CLIP_LM_PARAMS_INIT; dp_clip_lm_extra e = DP_CLIP_LM_EXTRA_INIT; ' \
           'return (int)(p.n_steps - 4 + e.reserved0); }\n'
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
        s.workspace_bytes = max(lib.dp_clip_lm_workspace_bytes(S, B) - short, 0)
        for key, v in k.items():
            setattr(s, key, v)
        return s

    def call(ctx, params=None, extra=None, result=None, b=batch, S=2, null=()):
        prm = params if params is not None else _lib.DpClipLmParams()
        ex = extra if extra is not None else ext(S if S > 0 else 2, b.n_frames if b.n_frames > 0 else 6)
        rs = result if result is not None else out
        rc = lib.dp_optimize_clip_lm(ctx, None if "batch" in null else C.byref(b), S, None if "params" in null else C.byref(prm), C.byref(rs),
                                     None if "extra" in null else C.byref(ex), None)
        return rc, (lib.dp_last_error(ctx).decode() if ctx else "")

    return call, ext, p, buf


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    call, ext, p, buf = _caller(lib)
    nan, inf = float("nan"), float("inf")
    assert call(None)[0] == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        for null in ("batch", "params", "extra"):
            rc, msg = call(ctx, null=(null,))
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
        # each stage names what it refuses, with a later stage's fault present as well
        stages = [(dict(params=prm(struct_size=36, n_steps=0)), "dp_clip_lm_params.struct_size is 36"),
                  (dict(params=prm(struct_size=5000, n_steps=0)), "dp_clip_lm_params.struct_size is 5000"),
                  (dict(result=small, params=prm(n_steps=0)), "dp_result.struct_size"),
                  (dict(extra=ext(struct_size=56), params=prm(n_steps=0)), "dp_clip_lm_extra.struct_size is 56"),
                  (dict(extra=ext(reserved0=1), params=prm(n_steps=0)), "reserved0 1"),
                  (dict(params=prm(n_steps=0, lambda_rot=nan)), "n_steps 0 outside 1..64"),
                  (dict(params=prm(n_steps=65, lambda_rot=nan)), "n_steps 65 outside 1..64"),
                  (dict(params=prm(lambda_rot=nan, mu_down=2.0)), "lambda_rot or lambda_tmp"),
                  (dict(params=prm(lambda_tmp=-1.0, mu_down=2.0)), "lambda_rot or lambda_tmp"),
                  (dict(params=prm(mu0=nan, mu_down=2.0)), "is not finite"),
                  (dict(params=prm(mu_max=inf, mu_down=2.0)), "is not finite"),
                  (dict(params=prm(mu_down=1.0, mu_up=1.0)), "mu_down must lie in (0, 1)"),
                  (dict(params=prm(mu_up=1.0, mu_min=2.0, mu_max=1.0)), "mu_up must be greater than 1"),
                  (dict(params=prm(mu_min=2.0, mu_max=1.0, mu0=5.0)), "0 < mu_min <= mu_max"),
                  (dict(params=prm(mu0=5e6), b=bad_batch), "mu0 outside [mu_min, mu_max]"),
                  (dict(b=bad_batch, S=0), "n_frames must be positive"),
                  (dict(b=null_batch, S=0), "NULL input array"),
                  (dict(S=0, params=prm(lambda_smooth=nan)), "n_sequences 0 must be positive and divide n_frames 6"),
                  (dict(S=-2, params=prm(lambda_smooth=nan)), "n_sequences -2 must be positive"),
                  (dict(S=4, params=prm(lambda_smooth=-1.0)), "n_sequences 4 must be positive and divide n_frames 6"),
                  (dict(params=prm(lambda_smooth=nan), extra=ext(workspace=None)), "lambda_smooth is negative or not finite"),
                  (dict(params=prm(lambda_smooth=-0.5), extra=ext(short=1)), "lambda_smooth is negative or not finite"),
                  (dict(params=prm(lambda_smooth=inf)), "lambda_smooth is negative or not finite"),
                  (dict(extra=ext(workspace=None)), "workspace is NULL"),
                  (dict(extra=ext(short=1)), f"fewer than the {lib.dp_clip_lm_workspace_bytes(2, 6)} of dp_clip_lm_workspace_bytes(2, 6)"),
                  (dict(extra=ext(S=1, B=3), S=3), "fewer than the")]
        for kw, word in stages:
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and "dp_optimize_clip_lm" in msg, (word, msg)
        # well-formed, every optional pointer given or NULL, S = 1 and S = B: refused only because there is no device
        bare = _lib.DpClipLmExtra(workspace=p)
        bare.workspace_bytes = lib.dp_clip_lm_workspace_bytes(2, 6)
        for kw in (dict(), dict(extra=bare), dict(S=1), dict(S=6), dict(S=3), dict(params=prm(n_steps=64, lambda_smooth=0.0)),
                   dict(extra=ext(short=-1000))):
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_DEVICE and "dp_optimize_clip_lm" in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_workspace_bytes_is_monotone_and_zero_for_what_the_call_refuses():
    lib = _lib.load()
    ws = lib.dp_clip_lm_workspace_bytes
    assert [ws(*a) for a in ((0, 6), (-1, 6), (2, 0), (2, -4), (4, 6), (7, 6))] == [0] * 6
    prev = 0
    for T in (1, 2, 3, 7, 33, 65, 240, 5052):
        for S in (1, 2, 5, 64):
            n = ws(S, S * T)
            assert n > 0 and n % 16 == 0
            # per frame: two latents, A | g, L^-1 | y, two loss rows, two coupling parts, the flags; per sequence: 32 bytes; 16-byte rounding of 13 parts
            per_frame, per_seq = 2 * 96 + 2 * 2400 + 2 * 16 + 2 * 8 + 4, 16 + 4 * 4
            assert S * T * per_frame + S * per_seq <= n <= S * T * per_frame + S * per_seq + 13 * 15, (S, T, n)
        assert ws(1, T) > prev
        prev = ws(1, T)
    assert ws(3, 6) < ws(3, 9) and ws(2, 6) != 0 and ws(1, 5052) < 2 ** 31
    # the byte counts themselves (n_sequences, n_frames): both calls size one list, dp_clip.h's, and a caller's allocation must keep fitting
    assert [ws(*a) for a in ((1, 1), (3, 9), (2, 130), (1, 5052))] == [5152, 45536, 655824, 25482368]


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    for sym in _lib.CLIP_LM_SYMBOLS:
        getattr(lib, sym).argtypes, getattr(lib, sym).restype = getattr(_lib.load(), sym).argtypes, getattr(_lib.load(), sym).restype
    call, ext, p, buf = _caller(lib)
    ctx = _host_ctx(lib)
    try:
        rc, msg = call(ctx)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in msg
        assert call(ctx, S=4)[0] == _lib.DP_ERR_INVALID  # (its argument checks come first)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_clip_check_refuses_what_the_library_would():
    ClipLM().check()
    ClipLM(steps=64, smooth=0.0, mu0=1.0, mu_min=1.0, mu_max=1.0).check()
    for kw, word in ((dict(steps=0), "steps 0 outside 1..64"), (dict(steps=65), "steps 65 outside 1..64"), (dict(steps=2.5), "outside 1..64"),
                     (dict(mu0=float("nan")), "mu0 is not finite"), (dict(mu_max=float("inf")), "mu_max is not finite"),
                     (dict(mu_down=1.0), r"mu_down must lie in \(0, 1\)"), (dict(mu_up=1.0), "mu_up must be greater than 1"),
                     (dict(mu_min=0.0), "0 < mu_min <= mu_max"), (dict(mu0=1e7), r"mu0 outside \[mu_min, mu_max\]"),
                     (dict(smooth=-1.0), "smooth is negative or not finite"), (dict(smooth=float("nan")), "smooth is negative or not finite"),
                     (dict(smooth=float("inf")), "smooth is negative or not finite")):
        with pytest.raises(ValueError, match=word):
            ClipLM(**kw).check()
    s = ClipLM(5, smooth=2.5).to_struct(2.0, 0.5)
    assert (s.n_steps, s.lambda_rot, s.lambda_tmp, s.lambda_smooth) == (5, 2.0, 0.5, 2.5) and s.struct_size == C.sizeof(_lib.DpClipLmParams)


def test_the_kernels_keep_their_budget(tmp_path):
    """hipcc -S with the build's flags: no spilled vector register, no scratch, and the LDS figures the headers state"""
    notes = _kernel_notes("dp_clip.hip", tmp_path)
    assert len(notes) == 3
    pick = lambda word: [n for name, n in notes.items() if word in name]
    rows, chain, decide = pick("dp_clip_rows_kernel"), pick("dp_clip_chain_kernel"), pick("dp_clip_decide_kernel")
    assert len(rows) == len(chain) == len(decide) == 1
    for n in rows + chain + decide:
        assert n["vspill"] == 0 and n["scratch"] == 0, n
    assert rows[0]["lds"] == ROWS_LDS and rows[0]["lds"] <= 160 * 1024, rows[0]
    assert rows[0]["vgpr"] <= 512 and rows[0]["agpr"] <= 256, rows[0]  # (one wave per SIMD, as dp_lm_kernel)
    assert chain[0]["lds"] == CHAIN_LDS and chain[0]["vgpr"] <= 512, chain[0]  # (a lone wave per workgroup)
    assert decide[0]["lds"] == 0 and decide[0]["vgpr"] <= 64, decide[0]
    for name in notes:  # tests/test_instantiation_coverage.py claims these patterns for the optimise kernels
        assert not re.search(r"dp_w4\w*_kernel|dp_w16_kernel|dp_lm\w*_kernel", name)
