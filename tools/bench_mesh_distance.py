#!/usr/bin/env python3
"""Cost of rnb_mesh_distance (include/rnb_mesh_distance.h) on one MI355X, and the error of rnb_mesh_simplify on the mesh of a trained model.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_clean.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh, colours) and cleaned (rnb_mesh_clean, largest, outward) once; for every N of --cells and both placements the cleaned device mesh
is simplified on N^3 cells over the unit box, and for every level of --levels the distance is measured on the device in both directions (fine -> simplified, simplified ->
fine): stats.ms over --rounds rounds, the first untimed, median and min .. max, with ms_grid (bounding box and cell lists) against the rest (validation and the
queries), n_pairs per sample, the grid, the peak workspace -- beside the extraction, cleaning and simplification ms of the same meshes -- and the error table: mean / rms
/ max per (resolution, N, placement), level 1. A resolution whose extraction fails for lack of memory is reported as such and skipped.

  python tools/bench_mesh_distance.py [--steps 2000] [--resolution 512 1024] [--cells 128 256 512] [--levels 0 1] [--rounds 3] [--out profiles/mesh_distance.json]

Prints one JSON line (and writes it to --out when given).
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
    ap.add_argument("--res", type=int, default=800, help="image resolution of the training views")
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--cells", type=int, nargs="*", default=[128, 256, 512], help="N of the simplification")
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--rounds", type=int, default=3)
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

    def extract(r):
        opt = _abi.MeshOptions()
        c._check(c.f.mesh_default_options(C.byref(opt)))
        opt.res[:] = [r, r, r]
        opt.attributes = _abi.MESH_ATTR_COLORS
        m, st = _abi.Mesh(), _abi.MeshStats()
        c._check(c.f.extract_mesh(c._h, None, C.byref(opt), C.byref(m), C.byref(st)))
        return m, st

    def clean(m):
        out, st = _abi.Mesh(), _abi.MeshCleanStats()
        c._check(c.f.mesh_clean(c._h, None, C.byref(m), C.byref(c._clean_options("largest", "outward")), C.byref(out), None, C.byref(st)))
        return out, st

    def simplify(m, n, placement):
        out, st = _abi.Mesh(), _abi.MeshSimplifyStats()
        opt = c._simplify_options(*c.simplify_grid((0, 0, 0), (1, 1, 1), n), placement)
        c._check(c.f.mesh_simplify(c._h, None, C.byref(m), C.byref(opt), C.byref(out), C.byref(st)))
        return out, st

    def spread(t):
        t = np.asarray(t[1:] if len(t) > 1 else t)  # the first round is untimed
        return dict(median=round(float(np.median(t)), 3), min=round(float(t.min()), 3), max=round(float(t.max()), 3))

    def distance(a, b, level):
        opt = c._distance_options(level=level)
        runs = [c._mesh_distance_device(a, b, opt, False, None) for _ in range(args.rounds)]
        last = runs[-1]
        n_queries = last["n_samples"] + last["n_verts_from_used"]
        return dict(ms=spread([x["ms"] for x in runs]), ms_grid=spread([x["ms_grid"] for x in runs]), ms_rest=spread([x["ms"] - x["ms_grid"] for x in runs]),
                    n_samples=last["n_samples"], pairs_per_sample=round(last["n_pairs"] / max(n_queries, 1), 2), dims=last["dims"], n_cell_entries=last["n_cell_entries"],
                    n_large=last["n_large"], peak_workspace=last["peak_workspace"], mean=last["mean"], rms=last["rms"], max=last["max"])

    results = []
    for r in args.resolution:
        try:
            m, est = extract(r)
        except Exception as e:  # e.g. no memory on a card that others use
            results.append(dict(resolution=r, skipped=str(e)[:200]))
            continue
        cm, cst = clean(m)
        c.f.mesh_free(c._h, C.byref(m))
        row = dict(resolution=r, extract_ms=round(est.ms, 2), clean_ms=round(cst.ms, 2), n_tris=cst.n_tris_out, cases=[])
        for n in args.cells:
            for placement in ("quadric", "mean"):
                sms = []
                for _ in range(args.rounds):
                    sm, sst = simplify(cm, n, placement)
                    sms.append(sst.ms)
                    if len(sms) < args.rounds:
                        c.f.mesh_free(c._h, C.byref(sm))
                case = dict(n=n, placement=placement, simplify_ms=spread(sms), n_tris_out=sst.n_tris_out, levels=[])
                try:
                    for level in args.levels:
                        case["levels"].append(dict(level=level, fine_to_simplified=distance(cm, sm, level), simplified_to_fine=distance(sm, cm, level)))
                except Exception as e:
                    case["failed"] = str(e)[:200]
                c.f.mesh_free(c._h, C.byref(sm))
                row["cases"].append(case)
                print(json.dumps(case), file=sys.stderr)
        c.f.mesh_free(c._h, C.byref(cm))
        results.append(row)

    res = dict(metric="mesh_distance_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, results=results)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    c.close()


if __name__ == "__main__":
    main()
