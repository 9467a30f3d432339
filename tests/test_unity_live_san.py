"""CPU: the plug-in's additions (include/dragposer_unity.h) under AddressSanitizer and UndefinedBehaviorSanitizer, in a stand-alone program.

tests/unity_san/main.cpp walks every new setter's refusals with each array in a heap block of exactly its size, latent_ar.bin files that are
truncated, of the wrong rank, dims, order or tensor count, or state a name length of 0xFFFFFFF0, the predictor beside a loaded temporal
model, and a well-formed drag_pose_present -- which ends in the library's "linked without dp_cons_live.hip" because no kernel unit is
linked, with the handle's state unchanged.  It links dp_unity.cpp and the library's host files against tests/host_san/fake_hip.cpp.  Built
with the host compiler, run as a child process: no GPU, nothing loaded into this interpreter."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

from test_host_san import CSRC, CXXFLAGS, ROOT, SAN

UNITS = [os.path.join(ROOT, "tests", "unity_san", "main.cpp"), os.path.join(ROOT, "tests", "host_san", "fake_hip.cpp")] + \
        [os.path.join(CSRC, f) for f in ("dp_unity.cpp", "dp_host.cpp", "dp_w16_host.cpp", "dp_temporal_host.cpp")]
DATA = os.path.join(ROOT, "dragposer_amd", "data")


def test_the_plugin_additions_under_sanitizers(tmp_path, golden_dir):
    cxx = os.environ.get("CXX", "g++")

    def compile_unit(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cxx] + CXXFLAGS + ["-c", src, "-o", obj], check=True, timeout=600)
        return obj

    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        objs = list(ex.map(compile_unit, UNITS))
    exe = str(tmp_path / "unity_san")
    subprocess.run([cxx] + SAN + ["-static-libasan", "-static-libubsan"] + objs + ["-o", exe], check=True, timeout=600)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_temporal_bin as X

    plain, temporal, scratch = tmp_path / "plain", tmp_path / "temporal", tmp_path / "files"
    for d in (plain, temporal, scratch):
        os.makedirs(d)
    for d in (plain, temporal):
        shutil.copy(os.path.join(DATA, "dragposer_model.bin"), d / "dragposer_model.bin")
    X.write(X.tensors_from(os.path.join(golden_dir, "sequ.npz")), str(temporal / "temporal.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    clip = os.path.join(ROOT, "tests", "data", "example_clip.bvh")
    r = subprocess.run([exe, clip, str(plain), str(temporal), str(scratch)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
