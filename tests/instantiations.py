"""Test helper: the table of every optimise-kernel instantiation the product library compiles, one row each.

tests/test_instantiation_coverage.py (CPU) holds the table to the kernel symbols of the built library's gfx950 code objects, and
tests/test_hip_instantiations.py (GPU) runs every row and asserts, through dp_debug_last_launch, that the row is what ran.  A new
instantiation without a row fails the CPU suite; a row without a GPU test cannot exist."""
import collections
import ctypes as C

UNIT_W4, UNIT_W4_BP, UNIT_W16 = 1, 2, 3  # dp_debug_last_launch's unit codes (dp_kernel.h: DP_UNIT_*)
UNIT_W4_BP_LV = 6                      # (4 and 5 are the per-frame-skeleton units: tests/skeleton_cases.py)
UNIT_NAMES = {UNIT_W4: "w4", UNIT_W4_BP: "w4_bp", UNIT_W16: "w16", UNIT_W4_BP_LV: "w4_bplv"}
KERNEL_NAMES = {UNIT_W4: "dp_w4_kernel", UNIT_W4_BP: "dp_w4_bp_kernel", UNIT_W4_BP_LV: "dp_w4_bplv_kernel"}

Inst = collections.namedtuple("Inst", "unit waves early seq long")

INSTANTIATIONS = (
    # dp_w4.hip (dense rows of layer 2) and dp_w4_bp.hip (body-part rows): 4 waves of 4 frames; fixed count, early stop, sequence, each also LONG
    Inst(UNIT_W4, 4, 0, 0, 0), Inst(UNIT_W4, 4, 0, 0, 1),
    Inst(UNIT_W4, 4, 1, 0, 0), Inst(UNIT_W4, 4, 1, 0, 1),
    Inst(UNIT_W4, 4, 1, 1, 0), Inst(UNIT_W4, 4, 1, 1, 1),
    Inst(UNIT_W4_BP, 4, 0, 0, 0), Inst(UNIT_W4_BP, 4, 0, 0, 1),
    Inst(UNIT_W4_BP, 4, 1, 0, 0), Inst(UNIT_W4_BP, 4, 1, 0, 1),
    Inst(UNIT_W4_BP, 4, 1, 1, 0), Inst(UNIT_W4_BP, 4, 1, 1, 1),
    # dp_w4_bp_lv.hip: the body-part layout's fixed-count optimising launches (the iteration loop once per loop version).  What every plain
    # fixed-count call of the body-part layout runs; dp_w4_bp.hip's two fixed-count rows above are left to dp_forward and the debug dump
    Inst(UNIT_W4_BP_LV, 4, 0, 0, 0), Inst(UNIT_W4_BP_LV, 4, 0, 0, 1),
    # dp_w16*.hip: one wave per SIMD (4 waves) or two (8 waves); fixed count or early stop, each also LONG
    Inst(UNIT_W16, 4, 0, 0, 0), Inst(UNIT_W16, 4, 0, 0, 1),
    Inst(UNIT_W16, 4, 1, 0, 0), Inst(UNIT_W16, 4, 1, 0, 1),
    Inst(UNIT_W16, 8, 0, 0, 0), Inst(UNIT_W16, 8, 0, 0, 1),
    Inst(UNIT_W16, 8, 1, 0, 0), Inst(UNIT_W16, 8, 1, 0, 1),
)


def symbol(inst):
    """the mangled name of the row's kernel: template <int NW, bool EARLY, bool SEQ, bool LONG> dp_w4_kernel / dp_w4_bp_kernel / dp_w4_bplv_kernel,
    template <int NW, int WPS, bool EARLY, bool LONG> dp_w16_kernel (WPS = waves per SIMD = NW / 4)"""
    b = lambda v: f"Lb{int(v)}E"
    if inst.unit == UNIT_W16:
        assert not inst.seq
        return f"_Z13dp_w16_kernelILi{inst.waves}ELi{inst.waves // 4}E{b(inst.early)}{b(inst.long)}Ev5KArgs"
    name = KERNEL_NAMES[inst.unit]
    return f"_Z{len(name)}{name}ILi{inst.waves}E{b(inst.early)}{b(inst.seq)}{b(inst.long)}Ev5KArgs"


def inst_id(inst):
    kind = "seq" if inst.seq else "early" if inst.early else "fixed"
    return f"{UNIT_NAMES[inst.unit]}-{inst.waves}w-{kind}{'-long' if inst.long else ''}"


def last_launch(opt):
    """what the LatentOptimizer's context launched last (dp_debug_last_launch), as a row of the table"""
    out = (C.c_int * 5)()
    assert opt.lib.dp_debug_last_launch(opt.ctx, out) == 0
    return Inst(*out)


def set_layout(opt, bp):
    """dp_debug_set_w4_layout: 0 dense, 1 body-part, -1 query; returns the layout in place, or an error code"""
    import torch

    torch.cuda.synchronize()
    return opt.lib.dp_debug_set_w4_layout(opt.ctx, bp)
