"""CPU: the library's host code under AddressSanitizer and UndefinedBehaviorSanitizer, in a stand-alone program.

tests/host_san/main.cpp drives dp_host.cpp, dp_w16_host.cpp, dp_encoder_host.cpp and dp_temporal_host.cpp -- the exception shell, every
packer on buffers of exactly the documented size, every sized struct of the C ABI in a heap block of exactly struct_size bytes, and the
create / destroy of the three handles with each allocation failing in turn -- linked against tests/host_san/fake_hip.cpp instead of the HIP
runtime and the kernel units.  Built with the host compiler, run as a child process: no GPU, nothing loaded into this interpreter.  What
is checked, case by case, is in main.cpp; every condition there is exact."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dragposer_amd", "csrc")
UNITS = [os.path.join(ROOT, "tests", "host_san", f) for f in ("main.cpp", "fake_hip.cpp")] + \
        [os.path.join(CSRC, f) for f in ("dp_host.cpp", "dp_w16_host.cpp", "dp_encoder_host.cpp", "dp_temporal_host.cpp")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CXXFLAGS = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + SAN


def test_host_code_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")

    def compile_unit(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cxx] + CXXFLAGS + ["-c", src, "-o", obj], check=True, timeout=600)
        return obj

    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        objs = list(ex.map(compile_unit, UNITS))
    exe = str(tmp_path / "host_san")
    # (no HIP runtime on the link line; the sanitizers' runtimes inside the program, so that it starts the same whatever the environment preloads)
    subprocess.run([cxx] + SAN + ["-static-libasan", "-static-libubsan"] + objs + ["-o", exe], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
