"""CPU: the gradient entry point of include/dragposer_grad.h -- header, binding, exports, argument checks and the kernel's register
budget.  No compute call is made here (the GPU side is tests/test_hip_vjp.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_grad.h")


def test_header_declares_the_grad_symbols_and_the_library_exports_them():
    declared = set(re.findall(r"^int\s+(dp_\w+)\s*\(", open(HDR).read(), flags=re.M))
    assert declared == set(_lib.GRAD_SYMBOLS)
    assert not set(_lib.GRAD_SYMBOLS) & set(_lib.PUBLIC_SYMBOLS)  # (dragposer.h declares nothing new)
    lib = _lib.load()
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert "dp_vjp.hip" in G.HIP_SOURCES


def test_grad_in_layout_matches_the_c_compiler(tmp_path):
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.DpGradIn) == 8 + 6 * ptr
    if shutil.which("gcc") is None:
        pytest.skip("no gcc: layout checked against the arithmetic above only")
    fields = ("struct_size", "reserved0", "pose", "disp", "world_disp", "world_rot", "pos", "rot")
    src = tmp_path / "grad.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_grad.h"\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(dp_grad_in));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_grad_in, {f}));\n' for f in fields)
                   + 'dp_grad_in g = DP_GRAD_IN_INIT; printf("%u %d\\n", g.struct_size, (g.pose != 0) + (int)g.reserved0);\nreturn 0; }\n')
    exe = tmp_path / "grad"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = subprocess.check_output([str(exe)]).decode().split()
    want = [str(C.sizeof(_lib.DpGradIn))] + [str(getattr(_lib.DpGradIn, f).offset) for f in fields] + [str(C.sizeof(_lib.DpGradIn)), "0"]
    assert got == want


def test_argument_errors_are_refused_before_any_device_is_touched():
    lib = _lib.load()
    g = _lib.DpGradIn()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    rc = lib.dp_forward_vjp(None, 1, p, p, C.byref(g), p, None, None, None)
    assert rc == _lib.DP_ERR_INVALID and b"ctx is NULL" in lib.dp_last_error(None)
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK and ctx.value  # a context with no device behind it
    try:
        def call(n=1, z=p, cur=p, gr=C.byref(g), dz=p):
            return lib.dp_forward_vjp(ctx, n, z, cur, gr, dz, None, None, None), lib.dp_last_error(ctx).decode()

        for n in (0, -3):
            rc, msg = call(n=n)
            assert rc == _lib.DP_ERR_INVALID and "n_frames" in msg
        for kw in (dict(z=None), dict(cur=None), dict(gr=None), dict(dz=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg, kw
        for size, res in ((0, 0), (8, 0), (C.sizeof(g) - 1, 0), (5000, 0), (C.sizeof(g), 7)):
            bad = _lib.DpGradIn()
            bad.struct_size, bad.reserved0 = size, res
            rc, msg = call(gr=C.byref(bad))
            assert rc == _lib.DP_ERR_INVALID and "struct_size" in msg, (size, res)
        rc, msg = call()  # well-formed: refused only because there is no device
        assert rc == _lib.DP_ERR_DEVICE, (rc, msg)
    finally:
        lib.dp_destroy(ctx)


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK
    try:
        g = _lib.DpGradIn()
        buf = (C.c_float * 64)()
        p = C.cast(buf, C.c_void_p)
        assert lib.dp_forward_vjp(ctx, 1, p, p, C.byref(g), p, None, None, None) == _lib.DP_ERR_UNSUPPORTED
    finally:
        lib.dp_destroy(ctx)


def test_vjp_kernel_keeps_its_register_budget(tmp_path):
    notes = _kernel_notes("dp_vjp.hip", tmp_path)
    (name, n), = [(k, v) for k, v in notes.items() if "dp_vjp_kernel" in k]
    assert not re.match(r"_Z\d+dp_w(?:4|4_bp|16)_kernel", name)
    assert n["vspill"] == 0 and n["scratch"] == 0, (name, n)
    assert n["lds"] <= 64 * 1024, (name, n)


def test_decode_fk_is_exported_and_has_no_cpu_path():
    import torch

    import dragposer_amd
    from dragposer_amd.autograd import OUTPUTS, decode_fk

    assert dragposer_amd.decode_fk is decode_fk
    assert OUTPUTS == ("pose", "disp", "world_disp", "world_rot", "pos", "rot")
    with pytest.raises(ValueError):
        decode_fk(None, torch.zeros(1, 24), torch.zeros(1, 4), outputs=("pos", "bogus"))
