"""User-defined constraint terms for the per-frame latent optimisation: include/dragposer_terms.h, dp_optimize_terms.  A `Terms` table
of up to 16 `Term`s, each a PLANE on a joint, a DISTANCE band between a joint and a joint or a point, or the ALIGNment of a joint axis
with a joint axis or a world direction, optionally scaled (and its point / direction replaced) per frame.  Used by
`LatentOptimizer.optimize_terms` and `DragPose.run(terms=...)`; semantics in the header's comment.  Whole-sequence launches
(`LatentOptimizer.optimize_sequence(terms=...)`, `DragPose.run_frames(terms=...)`: include/dragposer_sequence_constraints.h) take a
`per_frame` of [S,4], held for all frames, or [T,S,4], one row per frame."""
import math
from dataclasses import dataclass, field
from typing import Optional

from . import _lib

PLANE, DISTANCE, ALIGN = _lib.DP_TERM_PLANE, _lib.DP_TERM_DISTANCE, _lib.DP_TERM_ALIGN
ONE_SIDED, DROP_UP = _lib.DP_TERM_ONE_SIDED, _lib.DP_TERM_DROP_UP
MAX_TERMS = _lib.DP_MAX_TERMS
NJ = 22


def _vec(v, name):
    v = tuple(float(x) for x in v)
    if len(v) != 3:
        raise ValueError(f"Term.{name} must have 3 components")
    return v


@dataclass
class Term:
    """One row of the table (dp_term).  Build it with Term.plane / Term.distance / Term.align.  `per_frame`: None or a [B,4] fp32
    device tensor of rows (x, y, z, s) -- (x, y, z) replaces `point` (PLANE, point-DISTANCE) or `dir` (world ALIGN), s scales the weight
    for that frame (0: off); read by the kernel at launch time, so it may be rewritten between frames (or graph replays)."""
    type: int
    joint_a: int
    joint_b: int = -1
    flags: int = 0
    weight: float = 1.0
    point: tuple = (0.0, 0.0, 0.0)
    dir: tuple = (0.0, 1.0, 0.0)
    axis_a: tuple = (0.0, 0.0, 1.0)
    axis_b: tuple = (0.0, 0.0, 1.0)
    p0: float = 0.0
    p1: float = 0.0
    per_frame: Optional[object] = None

    @classmethod
    def plane(cls, joint, normal, point=(0.0, 0.0, 0.0), weight=1.0, one_sided=False, per_frame=None):
        """d = normal . (W_joint - point); T = d^2, or relu(-d)^2 with one_sided (the joint stays on the normal's side)"""
        return cls(PLANE, int(joint), -1, ONE_SIDED if one_sided else 0, float(weight), _vec(point, "point"), _vec(normal, "dir"),
                   per_frame=per_frame)

    @classmethod
    def distance(cls, joint_a, joint_b=None, point=None, lo=0.0, hi=0.0, weight=1.0, drop_up=False, per_frame=None):
        """q = |h(P_a - P_b)|^2 (joint_b) or |h(W_a - point)|^2; T = relu(q - hi^2) + relu(lo^2 - q).  lo = hi = 0: a soft pin"""
        if joint_b is not None and point is not None:
            raise ValueError("Term.distance: give joint_b or a point, not both")
        if joint_b is None and point is None and per_frame is None:
            raise ValueError("Term.distance: give joint_b, or a point (or a per-frame row)")
        return cls(DISTANCE, int(joint_a), -1 if joint_b is None else int(joint_b), DROP_UP if drop_up else 0, float(weight),
                   _vec(point if point is not None else (0.0, 0.0, 0.0), "point"), p0=float(lo), p1=float(hi), per_frame=per_frame)

    @classmethod
    def align(cls, joint_a, axis_a, joint_b=None, axis_b=None, dir=None, threshold=0.0, margin=0.0, weight=1.0, drop_up=False,
              per_frame=None):
        """u = h(G_a axis_a), v = h(G_b axis_b) or h(dir); T = 0 if |u| <= threshold, else (1 - min(1, u/|u| . v/|v| + margin))^2"""
        if joint_b is None and dir is None and per_frame is None:
            raise ValueError("Term.align: give joint_b and axis_b, or a world dir (or a per-frame row)")
        if joint_b is not None and axis_b is None:
            raise ValueError("Term.align: joint_b needs axis_b")
        return cls(ALIGN, int(joint_a), -1 if joint_b is None else int(joint_b), DROP_UP if drop_up else 0, float(weight),
                   dir=_vec(dir if dir is not None else (0.0, 1.0, 0.0), "dir"), axis_a=_vec(axis_a, "axis_a"),
                   axis_b=_vec(axis_b if axis_b is not None else (0.0, 0.0, 1.0), "axis_b"), p0=float(threshold), p1=float(margin),
                   per_frame=per_frame)

    @property
    def active(self):
        return self.weight != 0.0

    @property
    def needs_global_pos(self):
        return self.active and (self.type == PLANE or (self.type == DISTANCE and self.joint_b < 0))

    def check(self, i=0, n_points=0):
        """ValueError for what dp_optimize_terms refuses as DP_ERR_INVALID (the header's list).  `n_points`: the table's points
        (dragposer_amd.Points, include/dragposer_points.h), which a PLANE or DISTANCE term may name as 22 + k"""
        def bad(msg):
            raise ValueError(f"term {i}: {msg}")

        NJ = 22 + (int(n_points) if self.type in (PLANE, DISTANCE) else 0)

        if self.type not in (PLANE, DISTANCE, ALIGN):
            bad(f"unknown type {self.type}")
        if int(self.flags) & ~(ONE_SIDED | DROP_UP):
            bad(f"unknown flag bits {self.flags}")
        if not 0 <= self.joint_a < NJ:
            bad(f"joint_a {self.joint_a} outside 0..{NJ - 1}" + (": an ALIGN term cannot name a point" if self.type == ALIGN and n_points else ""))
        if not -1 <= self.joint_b < NJ:
            bad(f"joint_b {self.joint_b} outside -1..{NJ - 1}" + (": an ALIGN term cannot name a point" if self.type == ALIGN and n_points else ""))
        if self.type == PLANE and self.joint_b != -1:
            bad("a PLANE has no second joint")
        if not (math.isfinite(self.weight) and self.weight >= 0.0):
            bad("the weight is negative or not finite")
        vals = list(self.point) + list(self.dir) + list(self.axis_a) + list(self.axis_b) + [self.p0, self.p1]
        if not all(math.isfinite(float(x)) for x in vals):
            bad("a point, dir, axis, p0 or p1 is not finite")
        unit = lambda v: abs(math.sqrt(sum(float(x) ** 2 for x in v)) - 1.0) <= 1e-4
        if self.type == PLANE and not unit(self.dir):
            bad("the plane's normal is not unit length")
        if self.type == DISTANCE and not 0.0 <= self.p0 <= self.p1:
            bad("DISTANCE needs 0 <= lo <= hi")
        if self.type == ALIGN:
            if self.p0 < 0.0:
                bad("ALIGN's threshold is negative")
            if not any(self.axis_a) or (self.joint_b >= 0 and not any(self.axis_b)):
                bad("ALIGN's axis is zero")
            if self.joint_b < 0 and self.per_frame is None and not unit(self.dir):
                bad("ALIGN's world direction is not unit length")

    def to_struct(self, B=None, device=None, steps=None):
        """`steps` (a whole-sequence launch of that many frames): per_frame may also be [steps,B,4]"""
        t = _lib.DpTerm(type=int(self.type), joint_a=int(self.joint_a), joint_b=int(self.joint_b), flags=int(self.flags),
                        weight=float(self.weight), p0=float(self.p0), p1=float(self.p1))
        t.point[:], t.dir[:] = list(self.point), list(self.dir)
        t.axis_a[:], t.axis_b[:] = list(self.axis_a), list(self.axis_b)
        if self.per_frame is not None:
            import torch

            from .optimizer import _check

            shape = (steps, B, 4) if steps is not None and getattr(self.per_frame, "dim", lambda: 2)() == 3 else (B, 4)
            t.per_frame = _check(self.per_frame, "per_frame", shape, torch.float32, device)
        return t


@dataclass
class Terms:
    """The table (dp_terms): up to 16 terms and the up axis DROP_UP zeroes.  Terms() is the plain tracker loss.  `points`: a
    dragposer_amd.Points of up to 4 weighted joint combinations; a PLANE or DISTANCE term names point k as joint 22 + k
    (points.joint(k)), and the table then runs through the entry points of include/dragposer_points.h."""
    terms: list = field(default_factory=list)
    up_axis: int = 1
    points: Optional[object] = None

    @property
    def has_points(self):
        """the table runs through the entry points of include/dragposer_points.h (an empty Points too: n_points = 0, dp_optimize_terms' bits)"""
        return self.points is not None

    def __len__(self):
        return len(self.terms)

    @property
    def needs_global_pos(self):
        return any(t.needs_global_pos for t in self.terms)

    @classmethod
    def from_constraints(cls, c):
        """a dragposer_amd.Constraints as a table (zero weights left out).  Order: head_hips_forward, head_hips_colinear, the two
        feet_floor planes, the two hips_feet_colinear bands -- the reference's order of the sum (drag_pose.py:178-183)"""
        up = int(c.up_axis)
        e = [0.0, 0.0, 0.0]
        e[up] = 1.0
        ts = []
        if c.w_head_hips_forward != 0.0:
            ts.append(Term.align(c.head_joint, c.fwd_axis, c.hips_joint, c.fwd_axis, threshold=c.fwd_threshold, margin=c.fwd_margin,
                                 weight=c.w_head_hips_forward, drop_up=True))
        if c.w_head_hips_colinear != 0.0:
            ts.append(Term.distance(c.head_joint, c.hips_joint, weight=c.w_head_hips_colinear, drop_up=True))
        if c.w_feet_floor != 0.0:
            for j in c.floor_joints:
                ts.append(Term.plane(j, e, [c.floor_level * x for x in e], weight=c.w_feet_floor / 2.0, one_sided=bool(c.floor_one_sided)))
        if c.w_hips_feet_colinear != 0.0:
            for j in c.foot_joints:
                ts.append(Term.distance(c.hips_joint, j, lo=0.0, hi=c.feet_radius, weight=c.w_hips_feet_colinear, drop_up=True))
        return cls(ts, up)

    def check(self):
        if len(self.terms) > MAX_TERMS:
            raise ValueError(f"Terms: at most {MAX_TERMS} terms, got {len(self.terms)}")
        if self.up_axis not in (0, 1, 2):
            raise ValueError("Terms.up_axis must be 0, 1 or 2")
        if self.points is not None:
            self.points.check()
        for i, t in enumerate(self.terms):
            t.check(i, len(self.points) if self.points is not None else 0)

    def row_steps(self, B):
        """dp_seq_extra.row_step of a whole-sequence launch: floats between two frames' rows of each term's per_frame (0: [B,4], held)"""
        return [4 * B if t.per_frame is not None and t.per_frame.dim() == 3 else 0 for t in self.terms]

    def frames(self, t0, t1):
        """the table of frames t0..t1 of a clip: every [T,S,4] per_frame cut to those rows (a view), the rest shared"""
        from dataclasses import replace

        cut = lambda t: replace(t, per_frame=t.per_frame[t0:t1]) if t.per_frame is not None and t.per_frame.dim() == 3 else t
        return Terms([cut(t) for t in self.terms], self.up_axis, self.points)

    def to_struct(self, B, device, global_pos_ptr=None, loss_terms_ptr=None, steps=None):
        """-> (_lib.DpTerms, the DpTerm array it points to: keep both alive for the call).  `steps`: as Term.to_struct"""
        self.check()
        n = len(self.terms)
        arr = (_lib.DpTerm * max(n, 1))(*[t.to_struct(B, device, steps) for t in self.terms])
        s = _lib.DpTerms(n_terms=n, up_axis=int(self.up_axis))
        s.terms = _lib.C.cast(arr, _lib.C.c_void_p) if n else None
        s.global_pos = global_pos_ptr
        s.loss_terms = loss_terms_ptr
        return s, arr
