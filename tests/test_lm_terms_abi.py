"""CPU: dp_optimize_lm_terms (include/dragposer_lm_terms.h) -- the header against the binding, the refusals on a context without a device in
the header's order, and dp_lm_terms_kernel's register and LDS budget.  No compute call is made here (the GPU side is
tests/test_hip_lm_terms.py)."""
import ctypes as C
import os
import re

import __graft_entry__ as G
from dragposer_amd import Term, Terms, _lib
from test_build_quality import _kernel_notes
from test_host_san import ROOT
from test_sequence_constraints_abi import _host_ctx

HDR = os.path.join(ROOT, "include", "dragposer_lm_terms.h")
TERMS_LDS = 123920  # dp_lm_terms.h: TERMS_LDS_BYTES = dp_lm.h's 121 488 + the table's 1 408 + 4 waves x 256 bytes of rows


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == ["dp_optimize_lm_terms"] == list(_lib.LM_TERMS_SYMBOLS)
    assert hasattr(_lib.load(), "dp_optimize_lm_terms")
    assert "dp_lm_terms.hip" in G.HIP_SOURCES
    lds = re.search(r"static_assert\(TERMS_LDS_BYTES == (\d+)", open(os.path.join(G.CSRC, "dp_lm_terms.h")).read())
    assert int(lds.group(1)) == TERMS_LDS


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    batch = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    bad_batch = _lib.DpBatch(n_frames=0, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    out = _lib.DpResult(z=p)
    small = _lib.DpResult(z=p)
    small.struct_size = 8
    good = Terms([Term.plane(4, (0, 1, 0)), Term.distance(3, 7, lo=0.1, hi=0.2)] * 8)  # (16 terms)
    assert len(good) == _lib.DP_MAX_TERMS

    def table(terms=good, gp=p, **k):
        s, keep = terms.to_struct(4, None, gp, p)
        for key, v in k.items():
            setattr(s, key, v)
        return s, keep

    def prm(**k):
        s = _lib.DpLmParams()
        for key, v in k.items():
            setattr(s, key, v)
        return s

    def call(ctx, params=None, extra=None, result=None, b=batch, terms=None, null=()):
        prm_ = params if params is not None else _lib.DpLmParams()
        ex = extra if extra is not None else _lib.DpLmExtra(mu=p)
        ts, keep = terms if terms is not None else table()
        rc = lib.dp_optimize_lm_terms(ctx, None if "batch" in null else C.byref(b), None if "params" in null else C.byref(prm_),
                                      None if "terms" in null else C.byref(ts), C.byref(result if result is not None else out),
                                      None if "extra" in null else C.byref(ex), None)
        del keep
        return rc, (lib.dp_last_error(ctx).decode() if ctx else "")

    assert call(None)[0] == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        for null in ("batch", "params", "terms"):
            rc, msg = call(ctx, null=(null,))
            assert rc == _lib.DP_ERR_INVALID and "NULL batch, params or terms" in msg, msg
        bad_term = Terms([Term.plane(4, (0, 1, 0))])
        bad_term.terms[0].joint_a = 22
        object.__setattr__(bad_term, "check", lambda: None)
        object.__setattr__(bad_term.terms[0], "check", lambda *a, **k: None)
        bad_ex = _lib.DpLmExtra(mu=p)
        bad_ex.reserved0 = 1
        # each stage names what it refuses, with a later stage's fault present as well
        stages = [(dict(params=prm(struct_size=44), terms=table(n_terms=17)), "dp_lm_params.struct_size is 44"),
                  (dict(result=small, terms=table(n_terms=17)), "dp_result.struct_size"),
                  (dict(extra=bad_ex, terms=table(n_terms=17)), "reserved0 1"),
                  (dict(terms=table(struct_size=8), params=prm(n_steps=0)), "dp_terms"),
                  (dict(terms=table(n_terms=17), params=prm(n_steps=0)), "n_terms 17 outside 0..16"),
                  (dict(terms=table(up_axis=3), params=prm(n_steps=0)), "up_axis outside 0..2"),
                  (dict(terms=table(bad_term), params=prm(n_steps=0)), "term 0: joint_a 22 outside 0..21"),
                  (dict(terms=table(gp=None), params=prm(n_steps=0)), "global_pos is NULL while an active PLANE"),
                  (dict(params=prm(n_steps=0), b=bad_batch), "n_steps 0 outside 1..64"),
                  (dict(params=prm(mu_down=2.0), b=bad_batch), "mu_down must lie in (0, 1)"),
                  (dict(params=prm(mu0=5e6), b=bad_batch), "mu0 outside [mu_min, mu_max]"),
                  (dict(b=bad_batch), "n_frames must be positive")]
        for kw, word in stages:
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and "dp_optimize_lm_terms" in msg, (word, msg)
        for kw in (dict(), dict(null=("extra",)), dict(terms=table(Terms(), gp=None))):  # well-formed: refused only because there is no device
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_DEVICE and "dp_optimize_lm_terms" in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_the_kernel_keeps_its_budget(tmp_path):
    """hipcc -S with the build's flags: one kernel in the unit, no spilled vector register, no scratch, the LDS figure the header states"""
    notes = _kernel_notes("dp_lm_terms.hip", tmp_path)
    assert len(notes) == 1
    (name, n), = notes.items()
    assert "dp_lm_terms_kernel" in name
    assert n["vspill"] == 0 and n["scratch"] == 0, n
    assert n["lds"] == TERMS_LDS and n["lds"] <= 160 * 1024, n
    assert n["vgpr"] <= 512 and n["agpr"] <= 256, n
