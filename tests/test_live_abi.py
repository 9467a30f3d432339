"""CPU: dp_live_step (include/dragposer_live.h), dp_optimize_sequence_gaps for one step in one launch -- header, binding, exports, the order
of its refusals on a context without a device (n_steps 0 and 2 among them), the test-only library's refusal, both kernels' register and
LDS budget, and tools/export_latent_ar_bin.py's file against a numpy reader.  No compute call is made here (the GPU side is
tests/test_hip_live.py)."""
import ctypes as C
import os
import re
import struct
import sys

import numpy as np
import pytest

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)
from test_gaps_abi import HOLD_LDS, _gaps
from test_holds_abi import _holds, _terms
from test_latent_ar_abi import AR_LDS, _ar, _frames
from test_sequence_constraints_abi import _args, _host_ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_live.h")
NAME = "dp_live_step"
# as built (hipcc -S, the flags of __graft_entry__): vector registers of dp_live_kernel / dp_live_ar_kernel
VGPR = {"plain": 236, "ar": 241}


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == [NAME] == list(_lib.LIVE_SYMBOLS)
    lib = _lib.load()
    assert hasattr(lib, NAME) and lib.dp_live_step.argtypes == lib.dp_optimize_sequence_gaps.argtypes
    assert "dp_cons_live.hip" in G.HIP_SOURCES
    assert G.EXTRA_FLAGS.get("dp_cons_live.hip") == G.EXTRA_FLAGS.get("dp_cons_gap.hip")
    assert G.SCHED_OVERRIDE.get("dp_cons_live.hip", "x") == G.SCHED_OVERRIDE.get("dp_cons_gap.hip", "x")
    assert "#define DP_STATUS" not in text  # the status bits stay where they are (include/dragposer.h, include/dragposer_gaps.h)


@pytest.mark.parametrize("with_ar", (True, False))
def test_refusals_come_in_the_documented_order_before_any_device_is_touched(with_ar):
    lib = _lib.load()
    fn = getattr(lib, NAME)
    buf, p, _, prm, st, adj, res = _args()
    fr = _frames(p, z_tgt=None if with_ar else p, n_steps=1)
    own, keep = _terms()
    hs, keep_h = _holds(p)
    ar = _ar(p)
    ar_ref = C.byref(ar) if with_ar else None
    gs = _gaps(p)
    assert fn(None, 4, p, C.byref(fr), C.byref(prm), C.byref(own), C.byref(hs), ar_ref, C.byref(gs), None, C.byref(st), C.byref(adj), C.byref(res),
              None, None) == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        def call(n=4, latent=p, frames=C.byref(fr), params=C.byref(prm), ext=C.byref(own), holds=C.byref(hs), ar=ar_ref, gaps=C.byref(gs), sk=None,
                 state=C.byref(st), step=C.byref(adj), out=C.byref(res), extra=None):
            rc = fn(ctx, n, latent, frames, params, ext, holds, ar, gaps, sk, state, step, out, extra, None)
            return rc, lib.dp_last_error(ctx).decode()

        # 1. the NULL arguments
        for kw in (dict(n=0), dict(latent=None), dict(frames=None), dict(params=None), dict(ext=None), dict(gaps=None), dict(state=None), dict(out=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg and NAME in msg, kw
        # 2. n_steps other than 1, before everything the two-launch call checks -- with every later stage's fault present as well
        bad_prm = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        bad_prm.struct_size = 8
        bad_g = _gaps(p, max_hold=-1, decay=0.0, state=False)
        for n_steps in (0, 2, -1, 60):
            for kw in (dict(), dict(params=C.byref(bad_prm)), dict(gaps=C.byref(bad_g))):
                rc, msg = call(frames=C.byref(_frames(p, z_tgt=fr.z_tgt, n_steps=n_steps)), **kw)
                assert rc == _lib.DP_ERR_INVALID and f"n_steps is {n_steps}" in msg and NAME in msg, (n_steps, msg)
        # 3. dp_optimize_sequence_gaps' stages, under this call's name
        bad_res = _lib.DpSeqResults(hist_scratch=p)
        bad_res.reserved0 = 7
        bad_own = _lib.DpTerms()
        bad_own.struct_size = 8
        bad_hs, k2 = _holds(p)
        bad_hs.struct_size = 12
        bad_extra = _lib.DpSeqExtra()
        bad_extra.struct_size = 12
        bad_sk = _lib.DpSkeletonIn(offsets=p.value, stride=5)
        bad_adam = _lib.DpParams(n_iter=10, lr=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        stages = [(dict(params=C.byref(bad_prm)), "dp_params.struct_size"), (dict(out=C.byref(bad_res)), "dp_seq_results.struct_size"),
                  (dict(ext=C.byref(bad_own)), "dp_terms.struct_size"), (dict(holds=C.byref(bad_hs)), "dp_holds.struct_size"),
                  (dict(extra=C.byref(bad_extra)), "dp_seq_extra.struct_size"), (dict(sk=C.byref(bad_sk)), "dp_skeleton_in.stride"),
                  (dict(params=C.byref(bad_adam)), "Adam")]
        if with_ar:
            stages += [(dict(ar=C.byref(_lib.DpLatentAR(order=5))), "dp_latent_ar.order 5"), (dict(frames=C.byref(_frames(p, z_tgt=p, n_steps=1))), "z_tgt must be NULL")]
        else:
            stages += [(dict(frames=C.byref(_frames(p, z_tgt=None, n_steps=1))), "NULL input array")]
        for kw, word in stages:
            rc, msg = call(**{"gaps": C.byref(bad_g), **kw})
            assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (word, msg)
        for g, word in ((bad_g, "dp_gaps.max_hold -1"), (_gaps(p, decay=2.0, state=False), "dp_gaps.decay"), (_gaps(p, state=False), "dp_gaps.state is NULL")):
            rc, msg = call(gaps=C.byref(g))
            assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (word, msg)
        # well-formed: refused only because there is no device
        for kw in (dict(), dict(holds=None), dict(ext=C.byref(_lib.DpTerms()), holds=None), dict(gaps=C.byref(_gaps(p, max_hold=0, decay=1.0))),
                   dict(gaps=C.byref(_gaps(p, present=p, trace=p))), dict(extra=C.byref(_lib.DpSeqExtra())), dict(step=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_DEVICE and NAME in msg, (kw, rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del keep, keep_h, buf, k2


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        buf, p, _, prm, st, adj, res = _args()
        own, keep = _terms()
        ar, gs = _ar(p), _gaps(p)
        for fr, ar_ref in ((_frames(p, n_steps=1), C.byref(ar)), (_frames(p, z_tgt=p, n_steps=1), None)):
            rc = lib.dp_live_step(ctx, 4, p, C.byref(fr), C.byref(prm), C.byref(own), None, ar_ref, C.byref(gs), None, C.byref(st), C.byref(adj),
                                  C.byref(res), None, None)
            assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)


def test_both_kernels_keep_the_budget(tmp_path):
    """The in-kernel append adds no LDS: the kernel with the predictor has dp_terms_gap_ar_seq_kernel's AR_LDS_BYTES, exactly, the one without
    dp_terms_gap_seq_kernel's.  No spill, no scratch, at most 256 registers (two waves per SIMD, as the other sequence kernels); the counts
    as built are pinned so that a change shows."""
    notes = _kernel_notes("dp_cons_live.hip", tmp_path)
    assert len(notes) == 2
    by = {("ar" if "dp_live_ar_kernel" in k else "plain"): v for k, v in notes.items()}
    assert any("dp_live_kernel" in k for k in notes) and set(by) == {"ar", "plain"}
    assert by["ar"]["lds"] == AR_LDS == 79536 and by["plain"]["lds"] == HOLD_LDS <= AR_LDS
    for name, n in by.items():
        print(name, n)
        assert 2 * n["lds"] <= 160 * 1024
        assert n["vspill"] == 0 and n["scratch"] == 0, n
        assert n["vgpr"] + n["agpr"] <= 256, n
        assert n["vgpr"] == VGPR[name], n


def test_export_latent_ar_bin_round_trip(tmp_path):
    """LatentAR.save -> tools/export_latent_ar_bin.py -> a numpy reader of the DPM1 layout: the same bits"""
    from dragposer_amd import LatentAR

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_latent_ar_bin as X

    g = np.random.default_rng(11)
    ar = LatentAR(g.standard_normal((3, 24, 24)) * 0.1, g.standard_normal(24))
    src, dst = str(tmp_path / "ar.npz"), str(tmp_path / "latent_ar.bin")
    ar.save(src)
    X.write(X.tensors_from(src), dst)
    raw = open(dst, "rb").read()
    assert raw[:4] == b"DPM1" and struct.unpack_from("<I", raw, 4)[0] == 2
    at, got = 8, {}
    for _ in range(2):
        (n,) = struct.unpack_from("<I", raw, at)
        name = raw[at + 4:at + 4 + n].decode()
        (nd,) = struct.unpack_from("<I", raw, at + 4 + n)
        dims = struct.unpack_from(f"<{nd}I", raw, at + 8 + n)
        at += 8 + n + 4 * nd
        count = int(np.prod(dims))
        got[name] = np.frombuffer(raw, "<f4", count, at).reshape(dims)
        at += 4 * count
    assert at == len(raw) and list(got) == ["coeffs", "bias"]
    assert got["coeffs"].tobytes() == ar.A.tobytes() and got["bias"].tobytes() == ar.c.tobytes() and got["coeffs"].shape == (3, 24, 24)
    np.savez(str(tmp_path / "bad.npz"), A=np.zeros((2, 24, 23), np.float32), c=np.zeros(24, np.float32))
    with pytest.raises(ValueError, match="expected A"):
        X.tensors_from(str(tmp_path / "bad.npz"))
