"""CPU: dp_fit_bones' host code under AddressSanitizer and UndefinedBehaviorSanitizer, in a stand-alone program.

tests/fit_bones_san/main.cpp walks the call's refusals in the header's order with every sized struct in a heap block of exactly struct_size
bytes and `groups` / `base` / `prior` in blocks of exactly their sizes, linked with dp_host.cpp (and dp_w16_host.cpp, which dp_create needs)
against tests/host_san/fake_hip.cpp instead of the HIP runtime and the kernel units (so a well-formed call answers DP_ERR_UNSUPPORTED: the
launcher is a weak reference).  Built with the host compiler, run as a child process: no GPU, nothing loaded into this interpreter."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from test_host_san import CSRC, CXXFLAGS, ROOT, SAN

UNITS = [os.path.join(ROOT, "tests", "fit_bones_san", "main.cpp"), os.path.join(ROOT, "tests", "host_san", "fake_hip.cpp"),
         os.path.join(CSRC, "dp_host.cpp"), os.path.join(CSRC, "dp_w16_host.cpp")]  # (dp_create packs dp_w16's image)


def test_the_fit_bones_call_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")

    def compile_unit(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cxx] + CXXFLAGS + ["-c", src, "-o", obj], check=True, timeout=600)
        return obj

    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        objs = list(ex.map(compile_unit, UNITS))
    exe = str(tmp_path / "fit_bones_san")
    subprocess.run([cxx] + SAN + ["-static-libasan", "-static-libubsan"] + objs + ["-o", exe], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
