"""CPU: the additions of include/dragposer_unity.h for the live step (terms, holds, gaps, the latent AR predictor, drag_pose_present and the
read-backs): declared in the header, exported by libDragPoserDLL.so, and each setter's refusals that need no device -- its argument checks
first, then its own "call load_models first".  The GPU side is tests/test_hip_unity_live.py, the sanitized walk tests/unity_san/main.cpp
(run by tests/test_host_san.py)."""
import ctypes as C
import os
import re

from dragposer_amd import _lib
from test_unity_abi import CLIP, LIB, TEN, _load

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dragposer_unity.h")
NEW = ("drag_poser_set_terms", "drag_poser_set_holds", "drag_poser_set_gaps", "drag_poser_set_latent_ar", "drag_poser_load_latent_ar",
       "drag_pose_present", "drag_poser_last_status", "drag_poser_get_gap_codes", "drag_poser_get_hold_state")


def _bound():
    lib = _load()
    lib.drag_poser_set_terms.argtypes = [C.c_void_p, C.c_int, C.POINTER(_lib.DpTerm), C.c_int]
    lib.drag_poser_set_holds.argtypes = [C.c_void_p, C.c_int, C.POINTER(_lib.DpHold)]
    lib.drag_poser_set_gaps.argtypes = [C.c_void_p, C.c_int, C.c_float]
    lib.drag_poser_set_latent_ar.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.drag_poser_load_latent_ar.argtypes = [C.c_void_p, C.c_char_p]
    lib.drag_poser_last_status.argtypes = [C.c_void_p]
    return lib


def test_header_declares_the_additions_and_the_library_exports_them():
    text = open(HDR).read()
    declared = re.findall(r"^(?:void|int|const char\*|DragPoser\*)\s+(\w+)\s*\(", text, flags=re.M)
    assert declared[:10] == list(TEN)  # the reference's ten, in its order, untouched
    assert set(NEW) <= set(declared)
    lib = _load()
    for sym in NEW:
        assert hasattr(lib, sym), sym
    assert "max_hold 0, decay 1" in text  # the header states what runs when drag_poser_set_gaps was never called


def test_each_setter_checks_its_arguments_then_asks_for_load_models(tmp_path):
    lib = _bound()
    h = lib.init_drag_poser()
    err = lambda: lib.drag_poser_last_error(h).decode()
    lib.set_reference_skeleton(h, CLIP.encode())
    assert err() == ""
    terms = (_lib.DpTerm * 17)(*[_lib.DpTerm(type=_lib.DP_TERM_PLANE, joint_a=4, weight=1.0) for _ in range(17)])
    lib.drag_poser_set_terms(h, 17, terms, 1)
    assert "nTerms 17 outside 0..16" in err()
    lib.drag_poser_set_terms(h, 2, terms, 3)
    assert "upAxis 3 outside 0..2" in err()
    lib.drag_poser_set_terms(h, 2, terms, -1)
    assert "upAxis -1" in err()
    buf = (C.c_float * 4)()
    terms[1].per_frame = C.cast(buf, C.c_void_p)
    lib.drag_poser_set_terms(h, 2, terms, 1)
    assert "term 1: per_frame must be NULL" in err()
    terms[1].per_frame = None
    lib.drag_poser_set_terms(h, 2, terms, 1)
    assert err() == "drag_poser_set_terms: call load_models first"
    holds = (_lib.DpHold * 5)()
    lib.drag_poser_set_holds(h, 5, holds)
    assert "nHolds 5 outside 0..4" in err()
    lib.drag_poser_set_holds(h, 1, holds)
    assert err() == "drag_poser_set_holds: call load_models first"
    lib.drag_poser_set_gaps(h, 65536, 0.9)
    assert "maxHold 65536 outside 0..65535" in err()
    lib.drag_poser_set_gaps(h, 3, 0.0)
    assert "decay" in err()
    lib.drag_poser_set_gaps(h, 3, 0.9)
    assert err() == "drag_poser_set_gaps: call load_models first"
    A, c = (C.c_float * (4 * 576))(), (C.c_float * 24)()
    lib.drag_poser_set_latent_ar(h, 5, A, c)
    assert "order 5 outside 0..4" in err()
    lib.drag_poser_set_latent_ar(h, 2, None, c)
    assert "NULL coeffs or bias" in err()
    lib.drag_poser_set_latent_ar(h, 2, A, c)
    assert err() == "drag_poser_set_latent_ar: call load_models first"
    lib.drag_poser_load_latent_ar(h, str(tmp_path / "absent.bin").encode())
    assert "drag_poser_load_latent_ar: cannot open" in err()
    bad = tmp_path / "latent_ar.bin"
    bad.write_bytes(b"DPM1" + (1).to_bytes(4, "little") + (0xFFFFFFF0).to_bytes(4, "little") + b"coeffs")
    lib.drag_poser_load_latent_ar(h, str(bad).encode())
    assert "truncated" in err()
    assert lib.drag_poser_last_status(h) == 0
    lib.destroy_drag_poser(h)
