"""CPU: every optimise kernel the built library contains has a row in tests/instantiations.py -- and so a GPU test that runs it
(tests/test_hip_instantiations.py) -- and every row names a kernel that exists.  Read from the library's own gfx950 code objects.

"Optimise kernel" is every kernel whose name is dp_w4<anything>_kernel or dp_w16_kernel, whatever the unit that compiles it calls it (the
loop-version unit's dp_w4_bplv_kernel went unseen while the pattern listed the names it knew).  The per-frame-skeleton units' kernels are left
out by name: they have a table of their own (tests/skeleton_cases.py, held to the symbols by tests/test_skeleton_abi.py)."""
import os
import re
import shutil
import subprocess

import pytest

from instantiations import INSTANTIATIONS, symbol  # tests/instantiations.py
from skeleton_cases import SKEL_INSTANTIATIONS, skel_symbol  # tests/skeleton_cases.py

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
        found |= set(re.findall(r"\b(_Z\d+dp_w(?:4\w*?|16)_kernelI\w*)", syms))
    skeleton = {re.match(r"_Z\d+(\w+?_kernel)I", skel_symbol(i)).group(1) for i in SKEL_INSTANTIATIONS}
    assert skeleton == {"dp_w4sk_kernel", "dp_w4sk_bp_kernel"}
    return {s for s in found if re.match(r"_Z\d+(\w+?_kernel)I", s).group(1) not in skeleton}


def test_every_compiled_optimise_kernel_has_a_row_in_the_gpu_table(tmp_path):
    found = _optimise_kernels(tmp_path)
    table = [symbol(i) for i in INSTANTIATIONS]
    assert len(set(table)) == len(table)
    assert found == set(table), (sorted(found - set(table)), sorted(set(table) - found))
