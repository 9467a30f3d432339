"""CPU: dp_optimize_clip_lm_skeleton's and dp_optimize_lm_skeleton's host code under AddressSanitizer and UndefinedBehaviorSanitizer, in a
stand-alone program.

tests/clip_skeleton_san/main.cpp is linked with the library's host files against tests/host_san/fake_hip.cpp instead of the HIP runtime and
the kernel units, with the flags of tests/test_host_san.py, and run as a child process: no GPU, nothing loaded into this interpreter.  It
walks the two calls' refusals in the header's order -- the plain calls' own, dp_skeleton_in's, the workspace -- with every sized struct in a
heap block of exactly struct_size bytes; a well-formed call there answers DP_ERR_UNSUPPORTED because the launchers are weak references."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from test_host_san import CSRC, CXXFLAGS, REFUSALS, ROOT, SAN

PROGRAM = "clip_skeleton_san"


def test_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    sources = {unit: os.path.join(CSRC, unit + ".cpp") for unit in REFUSALS}
    sources["fake_hip"] = os.path.join(ROOT, "tests", "host_san", "fake_hip.cpp")
    sources[PROGRAM] = os.path.join(ROOT, "tests", PROGRAM, "main.cpp")

    def compile_unit(item):
        name, src = item
        obj = str(tmp_path / (name + ".o"))
        subprocess.run([cxx] + CXXFLAGS + ["-c", src, "-o", obj], check=True, timeout=600)
        return obj

    with ThreadPoolExecutor(max_workers=len(sources)) as ex:
        objects = list(ex.map(compile_unit, sources.items()))
    exe = str(tmp_path / PROGRAM)
    # (no HIP runtime on the link line; the sanitizers' runtimes inside the program, so that it starts the same whatever the environment preloads)
    subprocess.run([cxx] + SAN + ["-static-libasan", "-static-libubsan"] + objects + ["-o", exe], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("all checks held") == 2 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
