"""What tools/bench_mesh*.py have in common: the arguments all five take, the trained config-4 synthetic scene, the median and range of a list of times, and the JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arg_parser():
    """The parser with the arguments that come first in every tool's --help; the tool adds its own and hands it to parse_args."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--res", type=int, default=800, help="image resolution of the training views")
    return ap


def parse_args(ap):
    ap.add_argument("--out", default=None)  # the last one of every tool
    return ap.parse_args()


def train_scene(args):
    """The config-4 synthetic scene (args.views views of args.res x args.res) trained for args.steps steps -> (context, (views, normals, albedos), seconds of training)."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    scene = synthetic.make_scene(args.views, args.res)
    c = rnb.Context()
    c.init_params()
    c.set_dataset(*scene)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        c.train_step()
    return c, scene, time.perf_counter() - t0


def spread(times, prefix="", digits=3, untimed=1):
    """Median, min and max of `times` under prefix + "median" / "min" / "max"; the first `untimed` rounds are left out (unless nothing else was run)."""
    t = np.asarray(times[untimed:] if len(times) > untimed else times)
    return {prefix + "median": round(float(np.median(t)), digits), prefix + "min": round(float(t.min()), digits), prefix + "max": round(float(t.max()), digits)}


def report(res, out):
    """Print the result as one JSON line, and write it to `out` when given."""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
