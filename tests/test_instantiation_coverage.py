"""CPU: every optimise kernel the built library contains has a row in tests/instantiations.py -- and so a GPU test that runs it
(tests/test_hip_instantiations.py) -- and every row names a kernel that exists.  Read from the library's own gfx950 code objects."""
import os
import re
import shutil
import subprocess

import pytest

from instantiations import INSTANTIATIONS, symbol  # tests/instantiations.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dragposer_amd", "lib", "libdragposer_hip.so")


def _llvm_tool(name):
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    return p if os.path.exists(p) else shutil.which(name)


pytestmark = pytest.mark.skipif(_llvm_tool("llvm-objdump") is None or _llvm_tool("llvm-readelf") is None, reason="needs the ROCm LLVM tools")


def _optimise_kernels(tmp_path):
    lib = tmp_path / "libdragposer_hip.so"
    shutil.copy(LIB, lib)
    subprocess.check_call([_llvm_tool("llvm-objdump"), "--offloading", lib.name], cwd=tmp_path, stdout=subprocess.DEVNULL)
    objs = [p for p in tmp_path.iterdir() if p.name.startswith(lib.name + ".") and p.name.endswith("gfx950")]
    assert objs, sorted(p.name for p in tmp_path.iterdir())
    found = set()
    for co in objs:
        syms = subprocess.check_output([_llvm_tool("llvm-readelf"), "-s", "--wide", str(co)], text=True)
        found |= set(re.findall(r"\b(_Z\d+dp_w(?:4|4_bp|16)_kernel\w*)", syms))
    return found


def test_every_compiled_optimise_kernel_has_a_row_in_the_gpu_table(tmp_path):
    found = _optimise_kernels(tmp_path)
    table = [symbol(i) for i in INSTANTIATIONS]
    assert len(set(table)) == len(table)
    assert found == set(table), (sorted(found - set(table)), sorted(set(table) - found))
