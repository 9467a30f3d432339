"""Points (Effect): eval_drag --balance RADIUS:WEIGHT on a clip -- the centroid of all joints (uniform masses)
horizontally within RADIUS of the midpoint of joints 4 and 8 -- for the 3- and 4-tracker configurations, without it and at radii 0.05 /
0.1 / 0.2 and weights 0.1 / 1 / 10, alone and beside --constraints reference (y up, as that block has it).  One process; one RESULT line
per run: MPJPE, MPEEPE, iterations per frame and foot skate.
    python tools/points_effect.py tests/data/example_clip.bvh [--max-frames N]"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("clip")
    ap.add_argument("--max-frames", type=int, default=None)
    ap.add_argument("--trackers", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--reference", action="store_true", help="beside --constraints reference instead of alone")
    args = ap.parse_args()
    from dragposer_amd import eval_drag

    name = os.path.splitext(os.path.basename(args.clip))[0]
    settings = [None] + [(r, w) for w in (0.1, 1.0, 10.0) for r in (0.05, 0.1, 0.2)]
    with tempfile.TemporaryDirectory() as out:
        for n in args.trackers:
            cfg = os.path.join(ROOT, "dragposer_amd", "config", f"{n}_trackers_config.json")
            for s in settings:
                argv = [args.clip, "--config", cfg, "--out-dir", out, "--up-axis", "2", "--floor-level", "-1.0"]
                if args.max_frames is not None:
                    argv += ["--max-frames", str(args.max_frames)]
                if args.reference:
                    argv += ["--constraints", "reference"]
                # (weight 0 is the run without the term, through the same entry point, so that the skate line is printed for it too)
                argv += ["--balance", f"{s[0]}:{s[1]}" if s else "0.1:0"]
                with contextlib.redirect_stdout(io.StringIO()):
                    r = eval_drag.main(argv)[0]
                what = f"radius {s[0]:4.2f} weight {s[1]:4.1f}" if s else "none                   "
                print(f"RESULT {name:12s} {'reference + ' if args.reference else ''}trackers {n} {what}  MPJPE {r['mpjpe']:.5f}  MPEEPE {r['mpeepe']:.5f}  "
                      f"iters/frame {r['mean_iters']:.2f}  skate {r['foot_skate']:.6f}  frames {r['frames']}  time {r['time']:.2f}", flush=True)


if __name__ == "__main__":
    main()
