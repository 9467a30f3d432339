"""Tethers (Effect): eval_drag --tether on the knees and elbows (joints 2, 6, 16, 20) of a clip, for the 3-, 4- and
6-tracker configurations, weights 0 (inert: the run without tethers) / 0.1 / 1 / 10, HI 0 and 0.02, alpha 0 and 1.  One process; one
RESULT line per run: MPJPE, MPEEPE, iterations per frame, foot skate, jitter and the ground truth's own jitter.
    python tools/tether_effect.py tests/data/example_clip.bvh [--max-frames N]"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JOINTS = (2, 6, 16, 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("clip")
    ap.add_argument("--max-frames", type=int, default=None)
    ap.add_argument("--trackers", type=int, nargs="+", default=[3, 4, 6])
    args = ap.parse_args()
    from dragposer_amd import eval_drag

    name = os.path.splitext(os.path.basename(args.clip))[0]
    settings = [(0.0, 0.0, 0.0)] + [(w, hi, a) for w in (0.1, 1.0, 10.0) for hi in (0.0, 0.02) for a in (0.0, 1.0)]
    with tempfile.TemporaryDirectory() as out:
        for n in args.trackers:
            cfg = os.path.join(ROOT, "dragposer_amd", "config", f"{n}_trackers_config.json")
            for w, hi, a in settings:
                argv = [args.clip, "--config", cfg, "--out-dir", out, "--up-axis", "2", "--floor-level", "-1.0"]
                if args.max_frames is not None:
                    argv += ["--max-frames", str(args.max_frames)]
                for j in JOINTS:
                    argv += ["--tether", f"{j}:{hi}:{w}:{a}"]
                with contextlib.redirect_stdout(io.StringIO()):
                    r = eval_drag.main(argv)[0]
                print(f"RESULT {name:8s} trackers {n} weight {w:5.1f} hi {hi:4.2f} alpha {a:3.1f}  MPJPE {r['mpjpe']:.5f}  MPEEPE {r['mpeepe']:.5f}  "
                      f"iters/frame {r['mean_iters']:.2f}  skate {r['foot_skate']:.6f}  jitter {r['jitter']:.6f} (ground truth {r['jitter_gt']:.6f})  "
                      f"frames {r['frames']}  time {r['time']:.2f}", flush=True)


if __name__ == "__main__":
    main()
