"""CPU: the bone-fit call (include/dragposer_calibration.h) -- the header against the C compiler and the binding, the refusals of dp_fit_bones
on a context without a device in the header's order, the test-only library's refusal, what BoneGroups refuses, the two kernels' register
and LDS budget, and the version pin.  No compute call is made here (the GPU side is tests/test_hip_fit_bones.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G
from dragposer_amd import BoneGroups, _lib
from test_build_quality import _kernel_notes
from test_host_san import ROOT
from test_sequence_constraints_abi import _host_ctx

HDR = os.path.join(ROOT, "include", "dragposer_calibration.h")
FIT_FIELDS = ("struct_size", "reserved0", "n_groups", "ridge", "groups", "base", "prior", "workspace", "workspace_bytes")
RESULT_FIELDS = ("struct_size", "reserved0", "scales", "offsets", "normal", "rms", "info", "status")
FIT_LDS = 70704  # dp_fit.h: LDS_BYTES
PART_BYTES = 640 * 4  # dp_fit.h: PART_FLOATS floats per workgroup of 4 frames


def test_header_declares_the_calls_and_the_library_exports_them():
    text = open(HDR).read()
    assert re.findall(r"^(?:int|size_t)\s+(dp_\w+)\s*\(", text, flags=re.M) == list(_lib.CALIBRATION_SYMBOLS) == ["dp_fit_bones_workspace_bytes", "dp_fit_bones"]
    lib = _lib.load()
    for sym in _lib.CALIBRATION_SYMBOLS:
        assert hasattr(lib, sym)
    assert re.search(r"#define DP_FIT_MAX_GROUPS 24\b", text) and _lib.DP_FIT_MAX_GROUPS == 24
    assert re.search(r"#define DP_FIT_NO_FRAMES 1\b", text) and re.search(r"#define DP_FIT_SINGULAR 2\b", text)
    assert (_lib.DP_FIT_NO_FRAMES, _lib.DP_FIT_SINGULAR) == (1, 2)
    assert "dp_fit.hip" in G.HIP_SOURCES
    lds = re.search(r"static_assert\(WPB == 4 && LDS_BYTES == (\d+)", open(os.path.join(G.CSRC, "dp_fit.h")).read())
    assert int(lds.group(1)) == FIT_LDS
    assert "Not covered" in text and "per sequence" in text and "plug-in" in text
    assert lib.dp_version() == 510  # (the header is an addition: DP_VERSION stays)
    assert [lib.dp_fit_bones_workspace_bytes(n) for n in (-1, 0, 1, 4, 5, 4096)] == [0, 0, PART_BYTES, PART_BYTES, 2 * PART_BYTES, 1024 * PART_BYTES]


def test_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "fit.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_calibration.h"\nint main(void) {\n'
                   'printf("%zu %zu %d\\n", sizeof(dp_bone_fit), sizeof(dp_bone_fit_result), DP_FIT_MAX_GROUPS);\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_bone_fit, {f}));\n' for f in FIT_FIELDS)
                   + "".join(f'printf("%zu\\n", offsetof(dp_bone_fit_result, {f}));\n' for f in RESULT_FIELDS)
                   + 'dp_bone_fit f = DP_BONE_FIT_INIT;\ndp_bone_fit_result r = DP_BONE_FIT_RESULT_INIT;\n'
                   'printf("%u %u %d %.9g %d %d %d %d %zu\\n", f.struct_size, f.reserved0, f.n_groups, f.ridge, f.groups != 0, f.base != 0, f.prior != 0, '
                   'f.workspace != 0, f.workspace_bytes);\n'
                   'printf("%u %u %d %d %d %d %d %d\\n", r.struct_size, r.reserved0, r.scales != 0, r.offsets != 0, r.normal != 0, r.rms != 0, r.info != 0, '
                   'r.status != 0);\nreturn 0; }\n')
    exe = tmp_path / "fit"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpBoneFit), C.sizeof(_lib.DpBoneFitResult), _lib.DP_FIT_MAX_GROUPS] == [56, 56, 24]
    n = len(FIT_FIELDS)
    assert [int(x) for x in lines[1:1 + n]] == [getattr(_lib.DpBoneFit, f).offset for f in FIT_FIELDS] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    assert [int(x) for x in lines[1 + n:1 + n + len(RESULT_FIELDS)]] == [getattr(_lib.DpBoneFitResult, f).offset for f in RESULT_FIELDS] == [0, 4, 8, 16, 24, 32, 40, 48]
    f, r = _lib.DpBoneFit(), _lib.DpBoneFitResult()
    got = lines[-2].split()
    assert [int(x) for x in got[:3]] == [f.struct_size, f.reserved0, f.n_groups] == [56, 0, 1]
    assert C.c_float(float(got[3])).value == f.ridge == C.c_float(1e-3).value
    assert [int(x) for x in got[4:]] == [0, 0, 0, 0, 0] and (f.groups, f.base, f.prior, f.workspace, f.workspace_bytes) == (None, None, None, None, 0)
    assert [int(x) for x in lines[-1].split()] == [r.struct_size, 0, 0, 0, 0, 0, 0, 0] == [56, 0, 0, 0, 0, 0, 0, 0]


def _call_factory(lib):
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    limbs = BoneGroups.limbs()

    def call(ctx, groups=limbs.groups, K=3, base=None, prior=None, ridge=1e-3, n_frames=9, null=(), fit_kw=None, res_kw=None, ws_short=0):
        keep = [(C.c_int * 22)(*groups)]
        fit = _lib.DpBoneFit(n_groups=K, ridge=ridge)
        fit.groups = None if "groups" in null else C.cast(keep[0], C.c_void_p)
        for name, arr in (("base", base), ("prior", prior)):
            if arr is not None:
                a = np.ascontiguousarray(arr, dtype=np.float32)
                keep.append(a)
                setattr(fit, name, a.ctypes.data)
        fit.workspace = None if "workspace" in null else p
        fit.workspace_bytes = max(lib.dp_fit_bones_workspace_bytes(n_frames) - ws_short, 0)
        res = _lib.DpBoneFitResult(scales=None if "scales" in null else p, offsets=p, normal=p, rms=p, info=p, status=p)
        for s, kw in ((fit, fit_kw), (res, res_kw)):
            for key, v in (kw or {}).items():
                setattr(s, key, v)
        batch = _lib.DpBatch(n_frames=n_frames, z0=None if "z0" in null else p, z_tgt=None, cur_rot=p, tgt_pos=p, tgt_rot=None, w=p, tracked=p)
        rc = lib.dp_fit_bones(ctx, None if "batch" in null else C.byref(batch), None if "fit" in null else C.byref(fit),
                              None if "result" in null else C.byref(res), None)
        del keep
        return rc, (lib.dp_last_error(ctx).decode() if ctx else "")

    return call, buf


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    call, buf = _call_factory(lib)
    nan, inf = float("nan"), float("inf")
    assert call(None)[0] == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        g = list(BoneGroups.limbs().groups)
        alt = lambda ch: [ch.get(j, x) for j, x in enumerate(g)]
        no_spine = [0 if x == 1 else x for x in g]
        bad_base = np.full((22, 3), 0.1, np.float32)
        bad_base[7, 1] = nan
        # each stage names what it refuses, with a later stage's fault present as well
        stages = [(dict(null=("batch",), K=0), "NULL batch, fit or result"),
                  (dict(null=("fit",), K=0), "NULL batch, fit or result"),
                  (dict(null=("result",), K=0), "NULL batch, fit or result"),
                  (dict(fit_kw=dict(struct_size=48), res_kw=dict(struct_size=8)), "dp_bone_fit.struct_size is 48"),
                  (dict(fit_kw=dict(struct_size=5000), K=0), "dp_bone_fit.struct_size is 5000"),
                  (dict(fit_kw=dict(reserved0=2), K=0), "reserved0 2"),
                  (dict(res_kw=dict(struct_size=48), null=("scales",)), "dp_bone_fit_result.struct_size is 48"),
                  (dict(res_kw=dict(reserved0=1), K=0), "reserved0 1"),
                  (dict(null=("scales",), K=0), "scales is NULL"),
                  (dict(K=0, groups=alt({5: 9})), "n_groups 0 outside 1..24"),
                  (dict(K=25, null=("groups",)), "n_groups 25 outside 1..24"),
                  (dict(null=("groups",), ridge=nan), "groups is NULL"),
                  (dict(groups=alt({5: 3}), ridge=nan), "groups[5] is 3, outside -1..2"),
                  (dict(groups=alt({21: -2}), base=bad_base), "groups[21] is -2"),
                  (dict(groups=no_spine, base=bad_base), "group 1 owns no bone"),
                  (dict(base=bad_base, prior=[1.0, inf, 1.0]), "base holds a value that is not finite"),
                  (dict(prior=[1.0, inf, 1.0], ridge=-1.0), "prior holds a value that is not finite"),
                  (dict(prior=[nan, 1.0, 1.0], ridge=-1.0), "prior holds"),
                  (dict(ridge=-1e-3, null=("workspace",)), "ridge is negative or not finite"),
                  (dict(ridge=nan, null=("workspace",)), "ridge is negative or not finite"),
                  (dict(ridge=inf, n_frames=0), "ridge is negative or not finite"),
                  (dict(null=("workspace",), n_frames=0), "workspace is NULL"),
                  (dict(ws_short=1, null=("z0",)), "fewer than the 7680 of dp_fit_bones_workspace_bytes(9)"),
                  (dict(n_frames=0, null=("z0",)), "n_frames must be positive"),
                  (dict(n_frames=-3), "n_frames must be positive"),
                  (dict(null=("z0",)), "NULL input array")]
        for kw, word in stages:
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and "dp_fit_bones" in msg, (word, msg)
        # well-formed (z_tgt and tgt_rot NULL: not read; entry 0 of the groups ignored): refused only because there is no device
        for kw in (dict(), dict(base=np.full((22, 3), 0.1, np.float32), prior=[0.9, 1.0, 1.1]), dict(ridge=0.0), dict(groups=alt({0: 77})),
                   dict(groups=BoneGroups.per_bone().groups, K=21, n_frames=4096), dict(groups=BoneGroups.uniform().groups, K=1, n_frames=1)):
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_DEVICE and "dp_fit_bones" in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    for sym in ("dp_fit_bones", "dp_fit_bones_workspace_bytes"):
        getattr(lib, sym).argtypes, getattr(lib, sym).restype = getattr(_lib.load(), sym).argtypes, getattr(_lib.load(), sym).restype
    call, buf = _call_factory(lib)
    ctx = _host_ctx(lib)
    try:
        rc, msg = call(ctx)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in msg
        assert call(ctx, K=0)[0] == _lib.DP_ERR_INVALID  # (its argument checks come first)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_bone_groups_refuse_what_the_library_would():
    assert len(BoneGroups.uniform()) == 1 and len(BoneGroups.limbs()) == 3 and len(BoneGroups.symmetric()) == 13 and len(BoneGroups.per_bone()) == 21
    assert BoneGroups.limbs().members(1) == [9, 10, 11, 12, 13] and BoneGroups.symmetric().members(3) == [4, 8]
    assert BoneGroups([5] + [0] * 21).groups[0] == -1  # (entry 0 is ignored)
    for groups, word in (([0] * 21, "21 entries"), ([-1] + [-1] * 21, "0 groups"), ([-1] + [0] * 20 + [2], "group 1 owns no bone"),
                         ([-1] + [0] * 20 + [-2], r"groups\[21\] is -2"), ([-1] + list(range(21))[:-1] + [30], "31 groups")):
        with pytest.raises(ValueError, match=word):
            BoneGroups(groups)
    g = BoneGroups.limbs()
    for kw, word in ((dict(ridge=-1.0), "ridge is negative"), (dict(ridge=float("nan")), "ridge is negative or not finite"),
                     (dict(base=np.zeros((21, 3))), r"base must be \[22,3\]"), (dict(prior=[1.0, 1.0]), "prior must hold 3 values")):
        with pytest.raises(ValueError, match=word):
            g.to_struct(**kw)
    fit, keep = g.to_struct(base=np.ones((22, 3)), prior=[1, 2, 3], ridge=0.5)
    assert (fit.n_groups, fit.ridge, fit.struct_size) == (3, 0.5, C.sizeof(_lib.DpBoneFit)) and fit.groups and fit.base and fit.prior and len(keep) == 3


def test_the_kernels_keep_their_budget(tmp_path):
    """hipcc -S with the build's flags: no spilled vector register, no scratch, and the LDS figure the header states"""
    notes = _kernel_notes("dp_fit.hip", tmp_path)
    assert len(notes) == 2
    rows = [n for name, n in notes.items() if "dp_fit_rows_kernel" in name]
    solve = [n for name, n in notes.items() if "dp_fit_solve_kernel" in name]
    assert len(rows) == 1 and len(solve) == 1
    for n in rows + solve:
        assert n["vspill"] == 0 and n["scratch"] == 0, n
    assert rows[0]["lds"] == FIT_LDS and 2 * rows[0]["lds"] <= 160 * 1024, rows[0]
    assert rows[0]["vgpr"] <= 128 and solve[0]["vgpr"] <= 128, (rows, solve)  # (two workgroups of four waves per CU: a wave may hold 256)
    assert solve[0]["lds"] == 10608, solve[0]  # S [640] + H [25][25] + the quadratic forms' parts [48] in double, the scales [24]
    for name in notes:  # tests/test_instantiation_coverage.py claims these patterns for the optimise kernels
        assert not re.search(r"dp_w4\w*_kernel|dp_w16_kernel", name)
