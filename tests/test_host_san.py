"""CPU: the library's host code under AddressSanitizer and UndefinedBehaviorSanitizer, in stand-alone programs.

Each program under tests/*_san/ is a main.cpp linked with some of the library's host files against tests/host_san/fake_hip.cpp instead of
the HIP runtime and the kernel units.  host_san drives the exception shell, every packer on buffers of exactly the documented size, the
first sized structs of the C ABI and the create / destroy of the three handles with each allocation failing in turn; unity_san walks the
plug-in's additions (include/dragposer_unity.h); every other program walks one entry point's refusals in its header's order with every
sized struct in a heap block of exactly struct_size bytes, and a well-formed call there answers DP_ERR_UNSUPPORTED because the launcher is
a weak reference.  What is checked, case by case, is in each main.cpp; every condition there is exact.

Every source is compiled once per session with the host compiler, each program is linked from the objects it names in PROGRAMS and run as
a child process: no GPU, nothing loaded into this interpreter.  tests/host_san/san_support.h holds what the mains share."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dragposer_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CXXFLAGS = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + SAN
REFUSALS = ("dp_host", "dp_w16_host")  # (dp_create packs dp_w16's image)


def stage_unity(tmp_path):
    """unity_san's arguments: the BVH clip, a model folder without temporal.bin, one with it, a folder for the latent_ar.bin variants."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_temporal_bin as X

    plain, temporal, scratch = tmp_path / "plain", tmp_path / "temporal", tmp_path / "files"
    for d in (plain, temporal, scratch):
        os.makedirs(d)
    for d in (plain, temporal):
        shutil.copy(os.path.join(ROOT, "dragposer_amd", "data", "dragposer_model.bin"), d / "dragposer_model.bin")
    X.write(X.tensors_from(os.path.join(ROOT, "tests", "golden", "sequ.npz")), str(temporal / "temporal.bin"))
    return [os.path.join(ROOT, "tests", "data", "example_clip.bvh"), str(plain), str(temporal), str(scratch)]


# program (its main is tests/<program>/main.cpp): the library units it links, and what stages its arguments.  The weak launcher references
# resolve by what is on the link line, so a program links no more than it names here.
PROGRAMS = {
    "host_san": (("dp_host", "dp_w16_host", "dp_encoder_host", "dp_temporal_host"), None),
    "holds_san": (REFUSALS, None),
    "latent_ar_san": (REFUSALS, None),
    "gaps_san": (REFUSALS, None),
    "tethers_san": (REFUSALS, None),
    "points_san": (REFUSALS, None),
    "lm_san": (REFUSALS, None),
    "lm_terms_san": (REFUSALS, None),
    "lm_seq_san": (REFUSALS, None),
    "lm_seq_terms_san": (REFUSALS, None),
    "fit_bones_san": (REFUSALS, None),
    "unity_san": (("dp_unity", "dp_host", "dp_w16_host", "dp_temporal_host"), stage_unity),
}


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    """Every distinct source compiled once: {unit or program name: object file}."""
    out = tmp_path_factory.mktemp("san_objects")
    cxx = os.environ.get("CXX", "g++")
    sources = {unit: os.path.join(CSRC, unit + ".cpp") for units, _ in PROGRAMS.values() for unit in units}
    sources["fake_hip"] = os.path.join(ROOT, "tests", "host_san", "fake_hip.cpp")
    sources.update({program: os.path.join(ROOT, "tests", program, "main.cpp") for program in PROGRAMS})

    def compile_unit(item):
        name, src = item
        obj = str(out / (name + ".o"))
        subprocess.run([cxx] + CXXFLAGS + ["-c", src, "-o", obj], check=True, timeout=600)
        return name, obj

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return dict(ex.map(compile_unit, sources.items()))


@pytest.mark.parametrize("program", PROGRAMS)
def test_under_sanitizers(program, objects, tmp_path):
    units, stage = PROGRAMS[program]
    exe = str(tmp_path / program)
    # (no HIP runtime on the link line; the sanitizers' runtimes inside the program, so that it starts the same whatever the environment preloads)
    subprocess.run([os.environ.get("CXX", "g++")] + SAN + ["-static-libasan", "-static-libubsan"] +
                   [objects[name] for name in (program, "fake_hip") + units] + ["-o", exe], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + (stage(tmp_path) if stage else []), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
