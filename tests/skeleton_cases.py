"""The per-frame-skeleton kernels (dp_w4_skel.hip, dp_w4_bp_skel.hip: include/dragposer_skeleton.h) as a table: one row per compiled
instantiation, each run on the GPU by tests/test_hip_skeleton.py and held against the library's symbols by tests/test_skeleton_abi.py."""
from collections import namedtuple

UNIT_W4_SKEL, UNIT_W4_BP_SKEL = 4, 5  # dp_debug_last_launch's unit codes (dp_kernel.h: DP_UNIT_W4_SKEL, DP_UNIT_W4_BP_SKEL)
LAYOUT_OF_UNIT = {UNIT_W4_SKEL: 0, UNIT_W4_BP_SKEL: 1}  # dp_debug_set_w4_layout's argument that makes a context launch the unit

SkelInst = namedtuple("SkelInst", "unit waves early seq long")
SKEL_INSTANTIATIONS = tuple(SkelInst(u, 4, e, s, l) for u in (UNIT_W4_SKEL, UNIT_W4_BP_SKEL)
                            for e, s in ((0, 0), (1, 0), (1, 1)) for l in (0, 1))


def skel_symbol(inst):
    """template <int NW, bool EARLY, bool SEQ, bool LONG> dp_w4sk_kernel / dp_w4sk_bp_kernel"""
    b = lambda v: f"Lb{int(v)}E"
    name = "dp_w4sk_kernel" if inst.unit == UNIT_W4_SKEL else "dp_w4sk_bp_kernel"
    return f"_Z{len(name)}{name}ILi{inst.waves}E{b(inst.early)}{b(inst.seq)}{b(inst.long)}Ev5KArgs"


def skel_inst_id(inst):
    kind = "seq" if inst.seq else "early" if inst.early else "fixed"
    return f"{'w4sk' if inst.unit == UNIT_W4_SKEL else 'w4sk_bp'}-{kind}{'-long' if inst.long else ''}"


SCALED_CLIP_FACTOR = 1.12  # tests/golden/f1_clip6_scaled.npz: tests/data/example_clip.bvh with every OFFSET line scaled by this


def scaled_bvh_text(text, factor):
    """a BVH file's text with every OFFSET line (End Sites included) scaled by `factor`, printed %.6f; everything else byte for byte.  What
    tools/make_f1_goldens.py hands the reference's eval_drag for f1_clip6_scaled and what the test regenerates from the committed clip."""
    out = []
    for line in text.splitlines(keepends=True):
        tok = line.split()
        if tok and tok[0] == "OFFSET":
            ind = line[:len(line) - len(line.lstrip())]
            line = ind + "OFFSET " + " ".join(f"{float(v) * factor:.6f}" for v in tok[1:4]) + "\n"
        out.append(line)
    return "".join(out)
