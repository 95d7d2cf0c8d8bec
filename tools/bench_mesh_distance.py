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
import json
import sys

import mesh_bench_common as common


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--cells", type=int, nargs="*", default=[128, 256, 512], help="N of the simplification")
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--rounds", type=int, default=3)
    args = common.parse_args(ap)

    c, (views, normals, albedos), train_s = common.train_scene(args)

    def distance(a, b, level):
        runs = [a.distance_to(b, level=level) for _ in range(args.rounds)]
        last = runs[-1]
        n_queries = last["n_samples"] + last["n_verts_from_used"]
        return dict(ms=common.spread([x["ms"] for x in runs]), ms_grid=common.spread([x["ms_grid"] for x in runs]), ms_rest=common.spread([x["ms"] - x["ms_grid"] for x in runs]),
                    n_samples=last["n_samples"], pairs_per_sample=round(last["n_pairs"] / max(n_queries, 1), 2), dims=last["dims"], n_cell_entries=last["n_cell_entries"],
                    n_large=last["n_large"], peak_workspace=last["peak_workspace"], mean=last["mean"], rms=last["rms"], max=last["max"])

    results = []
    for r in args.resolution:
        try:
            m = c.extract_mesh_device(r, colors=True)
        except Exception as e:  # e.g. no memory on a card that others use
            results.append(dict(resolution=r, skipped=str(e)[:200]))
            continue
        with m:
            cm = m.clean("largest", "outward")
        with cm:
            row = dict(resolution=r, extract_ms=round(m.stats["ms"], 2), clean_ms=round(cm.stats["ms"], 2), n_tris=cm.stats["n_tris_out"], cases=[])
            for n in args.cells:
                for placement in ("quadric", "mean"):
                    sms = []
                    for k in range(args.rounds):
                        sm = cm.simplify(*c.simplify_grid((0, 0, 0), (1, 1, 1), n), placement=placement)
                        sms.append(sm.stats["ms"])
                        if k < args.rounds - 1:
                            sm.free()
                    with sm:  # the last round's
                        case = dict(n=n, placement=placement, simplify_ms=common.spread(sms), n_tris_out=sm.stats["n_tris_out"], levels=[])
                        try:
                            for level in args.levels:
                                case["levels"].append(dict(level=level, fine_to_simplified=distance(cm, sm, level), simplified_to_fine=distance(sm, cm, level)))
                        except Exception as e:
                            case["failed"] = str(e)[:200]
                    row["cases"].append(case)
                    print(json.dumps(case), file=sys.stderr)
        results.append(row)

    res = dict(metric="mesh_distance_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, results=results)
    common.report(res, args.out)
    c.close()


if __name__ == "__main__":
    main()
