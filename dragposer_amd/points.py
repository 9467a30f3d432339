"""Points for the term table: include/dragposer_points.h.  A `Point` is a weighted combination V = sum_j m_j P_j of the 22 joints'
positions whose coefficients sum to 1 -- the centre of mass, the midpoint of the feet or of the hands -- and a `Points` list of up to 4
of them goes into `Terms(terms, up_axis, points=...)`, whose PLANE and DISTANCE terms then name point k as joint `points.joint(k)` =
22 + k.  Such a table runs through dp_optimize_terms_points and its skeleton and sequence forms (`LatentOptimizer.optimize_terms`,
`optimize_sequence(terms=)`, `DragPose.run(terms=)`, `run_frames(terms=)`); it does not combine with holds, gaps, the latent predictor,
tethers or live steps."""
import math

from . import _lib

MAX_POINTS = _lib.DP_MAX_POINTS
NJ = 22


class Point:
    """One point: `coeffs` is a dict {joint: m} (the joints left out are 0) or 22 values.  The coefficients must be finite and sum to 1
    within 1e-4 (check())."""

    def __init__(self, coeffs):
        if isinstance(coeffs, dict):
            m = [0.0] * NJ
            for j, v in coeffs.items():
                if not 0 <= int(j) < NJ:
                    raise ValueError(f"Point: joint {j} outside 0..21")
                m[int(j)] += float(v)
        else:
            m = [float(v) for v in coeffs]
            if len(m) != NJ:
                raise ValueError(f"Point: {len(m)} coefficients, expected {NJ} (or a dict of joint: coefficient)")
        self.coeffs = tuple(m)

    @classmethod
    def midpoint(cls, a, b):
        """halfway between joints a and b"""
        return cls({int(a): 0.5, int(b): 0.5}) if int(a) != int(b) else cls({int(a): 1.0})

    @classmethod
    def centroid(cls, masses=None):
        """the mass-weighted mean of the joints; `masses`: 22 non-negative values, not all 0, normalised to sum 1 (None: uniform)"""
        w = [1.0] * NJ if masses is None else [float(x) for x in masses]
        if len(w) != NJ:
            raise ValueError(f"Point.centroid: {len(w)} masses, expected {NJ}")
        total = math.fsum(w)
        if not (all(math.isfinite(x) and x >= 0.0 for x in w) and total > 0.0):
            raise ValueError("Point.centroid: masses must be finite, non-negative and not all 0")
        return cls([x / total for x in w])

    def check(self, k=0):
        """ValueError for what dp_points refuses in a row"""
        if not all(math.isfinite(x) and abs(x) <= 3.0e38 for x in self.coeffs):
            raise ValueError(f"point {k}: a coefficient is not finite")
        total = math.fsum(self.coeffs)
        if not abs(total - 1.0) <= 1e-4:
            raise ValueError(f"point {k}: the coefficients sum to {total}, not to 1 within 1e-4")

    def __repr__(self):
        return "Point({" + ", ".join(f"{j}: {m:g}" for j, m in enumerate(self.coeffs) if m != 0.0) + "})"


class Points:
    """Up to 4 points (dp_points); point k is index 22 + k of the table it goes into."""

    def __init__(self, points=()):
        self.points = [p if isinstance(p, Point) else Point(p) for p in points]

    def __len__(self):
        return len(self.points)

    def joint(self, k):
        """the index a term names point k by"""
        if not 0 <= int(k) < len(self.points):
            raise ValueError(f"Points.joint: point {k} outside 0..{len(self.points) - 1}")
        return NJ + int(k)

    def check(self):
        if len(self.points) > MAX_POINTS:
            raise ValueError(f"Points: at most {MAX_POINTS} points, got {len(self.points)}")
        for k, p in enumerate(self.points):
            p.check(k)

    def to_struct(self):
        """-> (_lib.DpPoints, the host array it points to: keep both alive for the call)"""
        self.check()
        n = len(self.points)
        arr = (_lib.C.c_float * max(n * NJ, 1))(*[m for p in self.points for m in p.coeffs])
        s = _lib.DpPoints(n_points=n)
        s.coeff = _lib.C.cast(arr, _lib.C.c_void_p) if n else None
        return s, arr
