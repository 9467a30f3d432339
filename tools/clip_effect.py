"""The joint clip solver's effect (Effect): eval_drag --smooth on a clip for the 3-, 4- and 6-tracker configurations at a
few lambda_smooth, with and without an anchor.  One process; one RESULT line per run (each a single run): MPJPE, MPEEPE and jitter before and
after the second pass, the ground truth's own jitter, the accepted steps and the sequence's loss.
    python tools/clip_effect.py tests/data/example_clip.bvh [--max-frames N] [--solver lm:3]
--accel replaces the settings by those of DESIGN.md section 18a (eval_drag --smooth-accel): the acceleration term alone at lambda_accel 0.5, 5
and 50 and one mixed row, lambda_smooth 0.5 with lambda_accel 5, each with anchor 0 and 0.1."""
import argparse
import contextlib
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = ((0.5, 0.0), (5.0, 0.0), (50.0, 0.0), (5.0, 0.1), (50.0, 0.1))  # (lambda_smooth, anchor), 4 steps each
ACCEL_SETTINGS = tuple((ls, la, anchor) for anchor in (0.0, 0.1) for ls, la in ((0.0, 0.5), (0.0, 5.0), (0.0, 50.0), (0.5, 5.0)))  # (lambda_smooth, lambda_accel, anchor)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("clip")
    ap.add_argument("--max-frames", type=int, default=None)
    ap.add_argument("--trackers", type=int, nargs="+", default=[3, 4, 6])
    ap.add_argument("--solver", default=None, help="the first pass's solver, as eval_drag --solver (default: Adam)")
    ap.add_argument("--accel", action="store_true", help="the acceleration term's settings (ACCEL_SETTINGS) instead of the first-difference ones")
    args = ap.parse_args()
    from dragposer_amd import eval_drag

    name = os.path.splitext(os.path.basename(args.clip))[0]
    with tempfile.TemporaryDirectory() as out:
        for n in args.trackers:
            cfg = os.path.join(ROOT, "dragposer_amd", "config", f"{n}_trackers_config.json")
            for lam, accel, anchor in (ACCEL_SETTINGS if args.accel else tuple((ls, None, a) for ls, a in SETTINGS)):
                argv = [args.clip, "--config", cfg, "--out-dir", out, "--smooth", f"{lam}:4:{anchor}"] + (["--smooth-accel", str(accel)] if accel is not None else [])
                if args.max_frames is not None:
                    argv += ["--max-frames", str(args.max_frames)]
                if args.solver is not None:
                    argv += ["--solver", args.solver]
                with contextlib.redirect_stdout(io.StringIO()):
                    r = eval_drag.main(argv)[0]
                h = r["smooth_loss_hist"]
                accel_word = "" if accel is None else f" lambda_accel {accel:5.1f}"
                print(f"RESULT {name:12s} trackers {n} first pass {args.solver or 'adam':5s} lambda_smooth {lam:5.1f}{accel_word} anchor {anchor:4.2f}  MPJPE {r['mpjpe']:.5f} -> "
                      f"{r['mpjpe_smooth']:.5f}  MPEEPE {r['mpeepe']:.5f} -> {r['mpeepe_smooth']:.5f}  jitter {r['jitter']:.6f} -> {r['jitter_smooth']:.6f} "
                      f"(ground truth {r['jitter_gt']:.6f})  accepted {r['smooth_accepted']}/4  sequence loss {h[0]:.5g} -> {h[-1]:.5g}  frames {r['frames']}",
                      flush=True)


if __name__ == "__main__":
    main()
