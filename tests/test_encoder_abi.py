"""CPU: the pose encoder's C ABI (include/dragposer_encoder.h) -- header, binding, exports, the fold, the kernel's weight image and
its NumPy emulation, argument checks and the kernel's register / LDS budget.  The GPU side is tests/test_hip_encoder.py.

Tolerance: the project's own for the encoder against the real reference (tests/test_host_pipeline.py, tests/golden/enc.npz):
mu, logvar atol 2e-5 rtol 1e-5; latent atol 5e-5 rtol 1e-5."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G
import encoder_emu as EMU
from dragposer_amd import _lib
from dragposer_amd.model import DEFAULT_MODEL
from test_build_quality import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_encoder.h")
MU_TOL = dict(atol=2e-5, rtol=1e-5)
LATENT_TOL = dict(atol=5e-5, rtol=1e-5)
ROWS, COLS = (112, 72, 48, 48), (176, 112, 72, 48)


@pytest.fixture(scope="module")
def raw():
    return np.load(DEFAULT_MODEL)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "enc.npz"))


def numpy_fold(raw):
    """A_l = P_l (W_l * M_l), c_l = P_l b_l in fp64, summed in the order of the middle index, rounded to fp32 once"""
    A, c = [], []
    for l in range(3):
        W = raw[f"encoder.layers.{l}.0.weight"][..., 0].astype(np.float64) * raw[f"encoder.layers.{l}.0.mask"][..., 0].astype(np.float64)
        b = raw[f"encoder.layers.{l}.0.bias"].astype(np.float64)
        P = raw[f"encoder.layers.{l}.1.weight"].astype(np.float64)
        acc, cb = np.zeros((P.shape[0], W.shape[1])), np.zeros(P.shape[0])
        for j in range(P.shape[1]):
            acc += P[:, j:j + 1] * W[j:j + 1, :]
            cb += P[:, j] * b[j]
        A.append(acc.astype(np.float32))
        c.append(cb.astype(np.float32))
    A.append(np.concatenate([raw["encoder.f_mu.weight"], raw["encoder.f_logvar.weight"]]).astype(np.float32))
    c.append(np.concatenate([raw["encoder.f_mu.bias"], raw["encoder.f_logvar.bias"]]).astype(np.float32))
    return A, c


@pytest.fixture(scope="module")
def folded(raw):
    lib = _lib.load()
    model, keep = _lib.encoder_model(raw)
    f = _lib.DpEncoderFolded()
    assert lib.dp_fold_encoder(C.byref(model), C.byref(f)) == _lib.DP_OK, lib.dp_encoder_last_error(None)
    return f


def folded_arrays(f):
    A = [np.ctypeslib.as_array(getattr(f, n)).reshape(r, k) for n, r, k in zip(("A0", "A1", "A2", "Ah"), ROWS, COLS)]
    c = [np.ctypeslib.as_array(getattr(f, n)) for n in ("c0", "c1", "c2", "ch")]
    return A, c


@pytest.fixture(scope="module")
def image(folded):
    lib = _lib.load()
    n = lib.dp_debug_encoder_image(C.byref(folded), None, None, 0)
    assert n == EMU.IMG_WORDS
    img, tab = np.zeros(n, np.float32), np.zeros((n, 3), np.int32)
    assert lib.dp_debug_encoder_image(C.byref(folded), img.ctypes.data_as(_lib._f), tab.ctypes.data_as(_lib._i), n) == n
    return img, tab


def test_header_declares_the_encoder_symbols_and_the_library_exports_them():
    declared = set(re.findall(r"^(?:int|const char\*)\s+(dp_\w+)\s*\(", open(HDR).read(), flags=re.M))
    assert declared == set(_lib.ENCODER_SYMBOLS)
    assert not set(_lib.ENCODER_SYMBOLS) & set(_lib.PUBLIC_SYMBOLS)  # (dragposer.h declares nothing new)
    lib = _lib.load()
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert lib.dp_version() == 510
    assert "dp_encoder.hip" in G.HIP_SOURCES and "dp_encoder_host.cpp" in G.HIP_SOURCES


def test_struct_layouts_match_the_c_compiler(tmp_path):
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.DpEncoderModel) == ptr + 16 * ptr  # struct_size padded to a pointer, 4 x 3 + 4 pointers
    assert C.sizeof(_lib.DpEncoderFolded) == 4 * (112 * 176 + 112 + 72 * 112 + 72 + 48 * 72 + 48 + 48 * 48 + 48)
    if shutil.which("gcc") is None:
        pytest.skip("no gcc: layout checked against the arithmetic above only")
    mf = ("struct_size", "conv_w", "conv_mask", "conv_b", "pool_w", "f_mu_w", "f_mu_b", "f_logvar_w", "f_logvar_b")
    ff = ("A0", "c0", "A1", "c1", "A2", "c2", "Ah", "ch")
    src = tmp_path / "enc.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_encoder.h"\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(dp_encoder_model));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_encoder_model, {f}));\n' for f in mf)
                   + 'printf("%zu\\n", sizeof(dp_encoder_folded));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_encoder_folded, {f}));\n' for f in ff)
                   + 'dp_encoder_model m = DP_ENCODER_MODEL_INIT; printf("%u %d\\n", m.struct_size, m.f_mu_w != 0);\nreturn 0; }\n')
    exe = tmp_path / "enc"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = subprocess.check_output([str(exe)]).decode().split()
    want = ([str(C.sizeof(_lib.DpEncoderModel))] + [str(getattr(_lib.DpEncoderModel, f).offset) for f in mf]
            + [str(C.sizeof(_lib.DpEncoderFolded))] + [str(getattr(_lib.DpEncoderFolded, f).offset) for f in ff]
            + [str(C.sizeof(_lib.DpEncoderModel)), "0"])
    assert got == want


def test_fold_equals_the_fp64_fold_bit_for_bit(raw, folded):
    A, c = folded_arrays(folded)
    An, cn = numpy_fold(raw)
    for l in range(4):
        assert A[l].view(np.uint32).tolist() == An[l].view(np.uint32).tolist(), l
        assert c[l].view(np.uint32).tolist() == cn[l].view(np.uint32).tolist(), l
    assert np.count_nonzero(A[0]) < A[0].size  # the skeleton mask survives the fold


def test_fold_refuses_every_null_pointer_by_name(raw):
    lib = _lib.load()
    f = _lib.DpEncoderFolded()
    names = [f"{k}[{l}]" for l in range(3) for k in ("conv_w", "conv_mask", "conv_b", "pool_w")] + ["f_mu_w", "f_mu_b", "f_logvar_w", "f_logvar_b"]
    for name in names:
        model, keep = _lib.encoder_model(raw)
        if "[" in name:
            getattr(model, name[:-3])[int(name[-2])] = None
        else:
            setattr(model, name, None)
        assert lib.dp_fold_encoder(C.byref(model), C.byref(f)) == _lib.DP_ERR_INVALID, name
        assert name in lib.dp_encoder_last_error(None).decode(), name
    model, keep = _lib.encoder_model(raw)
    assert lib.dp_fold_encoder(C.byref(model), None) == _lib.DP_ERR_INVALID and b"out is NULL" in lib.dp_encoder_last_error(None)
    assert lib.dp_fold_encoder(None, C.byref(f)) == _lib.DP_ERR_INVALID and b"model is NULL" in lib.dp_encoder_last_error(None)
    model.struct_size -= 8
    assert lib.dp_fold_encoder(C.byref(model), C.byref(f)) == _lib.DP_ERR_INVALID and b"struct_size" in lib.dp_encoder_last_error(None)


def test_folded_network_in_fp64_meets_the_bar_on_the_reference(folded, golden):
    A, c = folded_arrays(folded)
    h = golden["pose"].astype(np.float64)
    for l in range(3):
        h = h @ A[l].astype(np.float64).T + c[l].astype(np.float64)
        h = np.where(h > 0, h, 0.2 * h)
    out = h @ A[3].astype(np.float64).T + c[3].astype(np.float64)
    np.testing.assert_allclose(out[:, :24], golden["mu"], **MU_TOL)
    np.testing.assert_allclose(out[:, 24:], golden["logvar"], **MU_TOL)


def test_image_unpacks_to_the_folded_network(folded, image):
    img, tab = image
    A, c = folded_arrays(folded)
    gotA = [np.zeros_like(a) for a in A]
    gotc = [np.zeros_like(b) for b in c]
    seenA = [np.zeros(a.shape, np.int32) for a in A]
    seenc = [np.zeros(b.shape, np.int32) for b in c]
    for w, (l, r, k) in enumerate(tab.tolist()):
        if l < 0:
            assert img[w] == 0.0, w  # every word that holds nothing is zero
        elif k < 0:
            gotc[l][r] = img[w]
            seenc[l][r] += 1
        else:
            gotA[l][r, k] = img[w]
            seenA[l][r, k] += 1
    for l in range(4):
        assert gotA[l].view(np.uint32).tolist() == A[l].view(np.uint32).tolist(), l
        assert gotc[l].view(np.uint32).tolist() == c[l].view(np.uint32).tolist(), l
        assert (seenA[l] == 1).all() and (seenc[l] == 1).all(), l  # every weight (the non-zero ones among them) and bias exactly once
    assert (tab[:, 0] >= 0).sum() == sum(a.size for a in A) + sum(b.size for b in c)
    assert img.size * 4 <= 160 * 1024


def test_emulation_of_the_kernels_walk_meets_the_bar(image, golden):
    mu, lv, z = EMU.emulate(image[0], golden["pose"], golden["eps"])
    np.testing.assert_allclose(mu, golden["mu"], **MU_TOL)
    np.testing.assert_allclose(lv, golden["logvar"], **MU_TOL)
    np.testing.assert_allclose(z, golden["latent"], **LATENT_TOL)
    assert EMU.emulate(image[0], golden["pose"][:3])[2].tolist() == mu[:3].tolist()  # no eps: latent = mu


def _gpu_present():
    import torch

    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_present(), reason="a GPU is present")
def test_create_without_a_gpu_has_no_cpu_fallback(raw):
    lib = _lib.load()
    model, keep = _lib.encoder_model(raw)
    h = C.c_void_p()
    assert lib.dp_encoder_create(C.byref(h), C.byref(model), 0) == _lib.DP_ERR_DEVICE
    assert not h.value and b"no CPU fallback" in lib.dp_encoder_last_error(None)


def test_argument_errors_are_refused_before_any_device_is_touched(raw):
    lib = _lib.load()
    err = lambda: lib.dp_encoder_last_error(None).decode()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    assert C.addressof(buf) % 16 == 0
    # dp_encoder_create: the model is checked before the device
    h = C.c_void_p()
    assert lib.dp_encoder_create(None, None, 0) == _lib.DP_ERR_INVALID
    assert lib.dp_encoder_create(C.byref(h), None, 0) == _lib.DP_ERR_INVALID and "model is NULL" in err()
    model, keep = _lib.encoder_model(raw)
    model.struct_size = 12
    assert lib.dp_encoder_create(C.byref(h), C.byref(model), 0) == _lib.DP_ERR_INVALID and "struct_size" in err()
    model, keep = _lib.encoder_model(raw)
    model.f_logvar_b = None
    assert lib.dp_encoder_create(C.byref(h), C.byref(model), 0) == _lib.DP_ERR_INVALID and "f_logvar_b" in err()
    assert lib.dp_encoder_destroy(None) == _lib.DP_ERR_INVALID
    assert lib.dp_encoder_geometry(None, None, None, None) == _lib.DP_ERR_INVALID
    # dp_encode on a NULL handle: the arguments are judged first, the handle last
    assert lib.dp_encode(None, 4, None, None, p, p, p, None, None) == _lib.DP_ERR_INVALID and "pose is NULL" in err()
    assert lib.dp_encode(None, -1, p, None, p, p, p, None, None) == _lib.DP_ERR_INVALID and "negative" in err()
    assert lib.dp_encode(None, 4, C.c_void_p(p.value + 4), None, p, p, p, None, None) == _lib.DP_ERR_INVALID and "aligned" in err()
    assert lib.dp_encode(None, 4, p, None, p, p, p, None, None) == _lib.DP_ERR_INVALID and "handle is NULL" in err()
    assert lib.dp_encode(None, 0, p, None, p, p, p, None, None) == _lib.DP_ERR_INVALID and "handle is NULL" in err()

    # dp_sequence_begin
    def state(history=60, n_heights=6):
        st = _lib.DpSeqState()
        st.global_pos = st.global_rot = st.latent_buf = st.disp_buf = st.heights_buf = p.value
        st.history, st.n_heights = history, n_heights
        return st

    def begin(st=None, pose=p, pos=p, rot=p, hts=p, latent=p, n=2):
        rc = lib.dp_sequence_begin(None, n, pose, None, pos, rot, hts, C.byref(st) if st is not None else None, latent, None, None)
        return rc, err()

    for kw, word in ((dict(st=None), "state is NULL"), (dict(st=state(n_heights=9)), "n_heights"), (dict(st=state(n_heights=-1)), "n_heights"),
                     (dict(st=state(history=0)), "history"), (dict(st=state(), pose=None), "pose is NULL"),
                     (dict(st=state(), pos=None), "init_global_pos"), (dict(st=state(), rot=None), "init_global_rot"),
                     (dict(st=state(), hts=None), "init_heights"), (dict(st=state(), latent=None), "latent is NULL"),
                     (dict(st=state(), n=-2), "negative"), (dict(st=state()), "handle is NULL")):
        rc, msg = begin(**kw)
        assert rc == _lib.DP_ERR_INVALID and word in msg, (kw, msg)
    st = state()
    st.disp_buf = None
    rc, msg = begin(st=st)
    assert rc == _lib.DP_ERR_INVALID and "NULL pointer in state" in msg


def test_encoder_kernel_keeps_its_budget(tmp_path):
    notes = _kernel_notes("dp_encoder.hip", tmp_path)
    (name, n), = [(k, v) for k, v in notes.items() if "dp_encoder_kernel" in k]
    assert n["vspill"] == 0 and n["scratch"] == 0, (name, n)
    assert EMU.IMG_WORDS * 4 <= n["lds"] <= 160 * 1024, (name, n)
    assert n["vgpr"] + n["agpr"] <= 256, (name, n)  # two wavefronts per SIMD (512-thread workgroups)
    text = (tmp_path / "dp_encoder.hip.s").read_text()
    assert text.count("v_mfma_f32_16x16x4_f32") == sum(t * s for t, s in zip(EMU.TILES, EMU.STEPS))  # 544: every block once, none through the VALU


def test_native_encoder_is_exported_and_has_no_cpu_path():
    import dragposer_amd
    from dragposer_amd.encoder import NativePoseEncoder

    assert dragposer_amd.NativePoseEncoder is NativePoseEncoder
    with pytest.raises(ValueError):
        NativePoseEncoder(device="cpu")
