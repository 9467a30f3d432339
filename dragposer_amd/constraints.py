"""The reference's extra loss terms (DragPose.loss, `# Additional Losses`, drag_pose.py:129-183) as parameters of
`LatentOptimizer.optimize_constrained` / `DragPose.run(constraints=...)`: include/dragposer_constraints.h, dp_optimize_constrained."""
import math
from dataclasses import dataclass, field

from . import _lib


@dataclass
class Constraints:
    """Weights (>= 0; 0 = the term is off) and the reference's Xsens defaults.  `Constraints()` has every weight 0 (the plain tracker
    loss); `Constraints.reference()` is the reference's block as written: all four terms with weight 1."""
    w_feet_floor: float = 0.0
    w_head_hips_forward: float = 0.0
    w_head_hips_colinear: float = 0.0
    w_hips_feet_colinear: float = 0.0
    floor_joints: tuple = (4, 8)
    foot_joints: tuple = (3, 7)
    head_joint: int = 13
    hips_joint: int = 0
    up_axis: int = 1
    floor_one_sided: bool = False  # relu(floor_level - height)^2: a ground plane that keeps the feet above the floor
    floor_level: float = 0.0
    fwd_axis: tuple = field(default=(0.0, 0.0, 1.0))
    fwd_threshold: float = 0.5
    fwd_margin: float = 0.2
    feet_radius: float = 0.2

    @classmethod
    def reference(cls, **kw):
        """drag_pose.py:129-183 un-commented: every term with weight 1"""
        return cls(**{"w_feet_floor": 1.0, "w_head_hips_forward": 1.0, "w_head_hips_colinear": 1.0, "w_hips_feet_colinear": 1.0, **kw})

    @property
    def needs_global_pos(self):
        return self.w_feet_floor != 0.0

    def to_struct(self, global_pos_ptr=None, loss_extra_ptr=None):
        """-> _lib.DpConstraints (ValueError for what the library would refuse as DP_ERR_INVALID)"""
        for n in ("w_feet_floor", "w_head_hips_forward", "w_head_hips_colinear", "w_hips_feet_colinear"):
            x = float(getattr(self, n))
            if not (math.isfinite(x) and x >= 0.0):
                raise ValueError(f"Constraints.{n} must be finite and >= 0, got {x}")
        for n in ("floor_joints", "foot_joints"):
            if len(getattr(self, n)) != 2:
                raise ValueError(f"Constraints.{n} must name two joints")
        c = _lib.DpConstraints()
        c.w_feet_floor, c.w_head_hips_forward = self.w_feet_floor, self.w_head_hips_forward
        c.w_head_hips_colinear, c.w_hips_feet_colinear = self.w_head_hips_colinear, self.w_hips_feet_colinear
        c.floor_joints[:] = [int(j) for j in self.floor_joints]
        c.foot_joints[:] = [int(j) for j in self.foot_joints]
        c.head_joint, c.hips_joint, c.up_axis = int(self.head_joint), int(self.hips_joint), int(self.up_axis)
        c.floor_one_sided = int(bool(self.floor_one_sided))
        c.floor_level = self.floor_level
        c.fwd_axis[:] = [float(x) for x in self.fwd_axis]
        c.fwd_threshold, c.fwd_margin, c.feet_radius = self.fwd_threshold, self.fwd_margin, self.feet_radius
        c.global_pos = global_pos_ptr
        c.loss_extra = loss_extra_ptr
        return c
