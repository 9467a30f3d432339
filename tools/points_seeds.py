"""CPU: the seeds of tests/test_hip_points.py::test_true_combinations_against_the_fp64_oracle.  For each case the fp64 oracle
(tests/points_oracle.py) is compared with its own fp32 run through exactly the test's comparison -- test_hip_constraints._compare with the
twin rule, rtol 2e-3 on loss_terms -- so a seed that passes here leaves the kernel the room an fp32 restatement needs and no more; the
term's activity and reach are printed beside it.  Usage: python tools/points_seeds.py [case=seed ...]   (no GPU)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import points_oracle as PO  # noqa: E402
import test_hip_constraints as HC  # noqa: E402
import test_hip_points as TP  # noqa: E402
from oracle import ref_torch as R  # noqa: E402


def main():
    seeds = dict(TP.SEEDS)
    for a in sys.argv[1:]:
        k, v = a.split("=")
        seeds[k] = int(v)
    m64, m32 = R.OracleModel(dtype=torch.float64), R.OracleModel(dtype=torch.float32)
    bad = 0
    for case, seed in seeds.items():
        b, gp = HC._inputs(m64, TP.B2, seed=seed)
        terms, i = TP.cases(TP.B2, "cpu")[case]
        ref = PO.optimize_terms(m64, b, terms, gp, TP.N2, lam_tmp=0.02)
        twin = PO.optimize_terms(m32, b, terms, gp, TP.N2, lam_tmp=0.02)
        err = np.linalg.norm(twin["pos"] - ref["pos"], axis=-1).max(1) * 1000.0
        lt = ref["loss_terms"][:, i]
        pos, rot = torch.from_numpy(ref["pos"]), torch.from_numpy(ref["rot"]).reshape(TP.B2, 22, 3, 3)
        reach = PO.joints_reached(terms, i, pos, rot, torch.from_numpy(gp).double()).numpy()
        try:
            TP.compare(twin, ref, m64, b, gp, terms, i)
            verdict = "ok"
        except AssertionError as e:
            verdict, bad = "FAILS: " + str(e)[:200], bad + 1
        print(f"{case:16s} seed {seed}: fp32 twin max {err.max():.4f} mm, {int((err > 0.05).sum())} frames beyond 0.05 mm; term active in "
              f"{int((lt > 0).sum())}/{TP.B2} frames, sum {lt.sum():.4f}, joints reached {reach[lt > 0].min() if (lt > 0).any() else 0}"
              f"..{reach.max()}: {verdict}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
