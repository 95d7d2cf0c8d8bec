#!/usr/bin/env python3
"""Cost of the inference tracer (include/rnb_render.h) on one MI355X.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process, renders all 64 views with the EMA weights, and reports ms per frame,
rays/s and network samples/s. In the same process it then times one rnb_forward_infer call on as many random coordinates as a frame's marches wrote
(forward_infer_ms_random_coords). That is not the render's network work -- the rounds also evaluate the neutral padding records, and random coordinates
touch the hash grid differently -- so it is not subtracted from the frame time: the split between the network and the tracer around it comes from the
kernel trace (rocprofv3 --kernel-trace, profiles/render_kernel_stats.md).

  python tools/bench_render.py [--steps 2000] [--views 64] [--res 800] [--repeat 3] [--out profiles/render_bench.json]

Prints one JSON line (and writes it to --out when given). For the per-kernel table run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--repeat", type=int, default=3, help="timed passes over all views (the first, untimed, pass grows the workspace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic, _abi

    views, normals, albedos = synthetic.make_scene(args.views, args.res)
    c = rnb.Context()
    c.init_params()
    c.set_dataset(views, normals, albedos)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        c.train_step()
    train_s = time.perf_counter() - t0

    h, w = args.res, args.res
    n_px = h * w
    out = c.device_malloc(n_px * rnb.RENDER_CHANNELS * 4)
    for v in views:  # untimed pass: workspace allocation, code objects
        c.render_into(v, out)
    frame_ms, samples, rounds, hits = [], [], [], []
    t0 = time.perf_counter()
    for _ in range(args.repeat):
        for v in views:
            st = c.render_into(v, out)
            frame_ms.append(st["ms"])
            samples.append(st["n_samples"])
            rounds.append(st["rounds"])
            hits.append(st["n_hit"])
    wall = time.perf_counter() - t0
    n_frames = args.repeat * len(views)
    ms = wall * 1e3 / n_frames
    mean_samples = float(np.mean(samples))

    # one rnb_forward_infer call (EMA weights) on as many random coordinates as a mean frame's marches wrote, from device memory, same process
    n_eval = int(mean_samples)
    rng = np.random.default_rng(0)
    coords = np.empty((n_eval, 7), np.float32)
    coords[:, 0:3] = rng.uniform(0.3, 0.7, (n_eval, 3))  # inside the object's box, as the rendered samples are
    coords[:, 3] = 0.0
    coords[:, 4:7] = rng.uniform(0.0, 1.0, (n_eval, 3))
    cptr = c.upload(coords)
    optr = c.device_malloc(n_eval * 32)
    one = np.zeros(1, np.uint32)

    def sync():
        c._check(c.f.memcpy(c._h, one.ctypes.data_as(C.c_void_p), C.c_void_p(optr), 4, _abi.D2H))

    for _ in range(3):
        c._check(c.f.forward_infer(c._h, None, C.c_void_p(cptr), n_eval, C.c_void_p(optr), 1))
    sync()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        c._check(c.f.forward_infer(c._h, None, C.c_void_p(cptr), n_eval, C.c_void_p(optr), 1))
    sync()
    net_ms = (time.perf_counter() - t0) * 1e3 / reps
    c.device_free(cptr)
    c.device_free(optr)
    c.device_free(out)

    res = dict(metric="render_ms_per_frame", value=round(ms, 3), unit="ms/frame", res=[w, h], views=len(views), train_steps=args.steps, train_s=round(train_s, 2),
               rays_per_s=round(n_px / (ms * 1e-3)), samples_per_s=round(mean_samples / (ms * 1e-3)), samples_per_frame=round(mean_samples),
               rounds_per_frame=round(float(np.mean(rounds)), 2), hit_fraction=round(float(np.mean(hits)) / n_px, 4),
               frame_ms_median=round(float(np.median(frame_ms)), 3), forward_infer_ms_random_coords=round(net_ms, 3))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    c.close()


if __name__ == "__main__":
    main()
