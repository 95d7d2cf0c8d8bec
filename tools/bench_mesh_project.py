#!/usr/bin/env python3
"""Cost of rnb_mesh_project_views (include/rnb_mesh_project.h) on one MI355X, beside a per-pixel pass over the same fills and beside the model's own bake.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_raster.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh) and cleaned (rnb_mesh_clean, largest, outward) once, and simplified (quadric placement) on N^3 cells for every N of --cells. With
--full the cleaned mesh itself is measured too. Every one of these device meshes is textured from the scene's 64 albedo maps (uint16, as the loader reads them) at every S
of --size: ms per call (stats.ms: the median of --repeat calls after one untimed call, and min .. max), the textured fraction, the pairs tested and occluded.

Beside it, on the same mesh: DeviceMesh.visibility over the same 64 views (the same 64 fills with a per-pixel pass instead of a per-texel one) and DeviceMesh.bake_texture
at the same S (a network evaluation per texel instead of 64 projections). `beyond_fills_ms` = project - visibility is an estimate of what the per-texel passes cost: the
call does not time its phases, and the public interface has no fill on its own.

For the first mesh and the first size: n_textured / n_texels over --tolerances x --min-cos (the evidence for the two defaults), and the mean absolute difference between
the projected map and the model's baked albedo over the textured texels.

  python tools/bench_mesh_project.py [--steps 2000] [--resolution 512] [--cells 128 256] [--full] [--size 1024 2048 4096] [--repeat 3] [--out profiles/mesh_project.json]

Prints one JSON line (and writes it to --out when given). profiles/mesh_project.md is written by hand from that line, as the other profiles are.
"""
import json
import sys

import numpy as np

import mesh_bench_common as common


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512])
    ap.add_argument("--cells", type=int, nargs="*", default=[128, 256], help="N of the simplifications")
    ap.add_argument("--full", action="store_true", help="also the cleaned mesh without simplification")
    ap.add_argument("--size", type=int, nargs="*", default=[1024, 2048, 4096], help="texels per side")
    ap.add_argument("--tolerances", type=float, nargs="*", default=[2.0 ** -10, 2.0 ** -8, 2.0 ** -6])
    ap.add_argument("--min-cos", type=float, nargs="*", default=[0.0, 0.1, 0.3])
    ap.add_argument("--repeat", type=int, default=3)
    args = common.parse_args(ap)

    from rnb_neus2_amd import api

    c, (views, _, albedos), train_s = common.train_scene(args)
    images = [np.asarray(a).reshape(v["height"], v["width"], 4) for v, a in zip(views, albedos)]
    table = []

    def measure(name, m):
        rows = []
        vis = common.spread([m.visibility(views)[1]["ms"] for _ in range(args.repeat + 1)])
        for size in args.size:
            try:
                lay = api.Context.texture_layout(m.n_triangles, size)
                runs = [m.project_views(views, images, size=size)["stats"] for _ in range(args.repeat + 1)]
            except api.RnbError as e:
                rows.append(dict(mesh=name, n_tris=m.n_triangles, size=size, skipped=str(e)[-120:]))
                print(json.dumps(rows[-1]), file=sys.stderr)
                continue
            ms, st = common.spread([r["ms"] for r in runs]), runs[-1]
            bake = common.spread([m.bake_texture(size)["stats"]["ms"] for _ in range(args.repeat + 1)])
            rows.append(dict(mesh=name, n_tris=m.n_triangles, size=size, block=lay["block"], n_texels=st["n_texels"], textured=round(st["n_textured"] / max(st["n_texels"], 1), 4),
                             n_pairs_tested=st["n_pairs_tested"], n_occluded=st["n_occluded"], project_ms=ms, visibility_ms=vis, bake_ms=bake,
                             beyond_fills_ms=round(ms["median"] - vis["median"], 3), ns_per_texel_view=round((ms["median"] - vis["median"]) * 1e6 / max(st["n_texels"] * len(views), 1), 4),
                             peak_workspace=st["peak_workspace"]))
            print(json.dumps(rows[-1]), file=sys.stderr)
        if not table:  # the defaults' evidence, once
            size = args.size[0]
            baked = m.bake_texture(size)["albedo"]
            for tol in args.tolerances:
                for mc in args.min_cos:
                    r = m.project_views(views, images, size=size, depth_tolerance=tol, min_cos=mc)
                    seen = r["info"][..., 0] > 0
                    table.append(dict(mesh=name, size=size, depth_tolerance=tol, min_cos=mc, textured=round(r["stats"]["n_textured"] / max(r["stats"]["n_texels"], 1), 5),
                                      n_occluded=r["stats"]["n_occluded"], mean_abs_diff_to_model=round(float(np.abs(r["color"][seen][:, :3] - baked[seen][:, :3]).mean()), 5) if seen.any() else None))
                    print(json.dumps(table[-1]), file=sys.stderr)
        return rows

    results = []
    for r in args.resolution:
        with c.extract_mesh_device(r) as m:
            cm = m.clean("largest", "outward")
        with cm:
            block = dict(resolution=r, extract_ms=round(m.stats["ms"], 2), clean_ms=round(cm.stats["ms"], 2), calls=[])
            for n in args.cells:
                with cm.simplify(*c.simplify_grid((0, 0, 0), (1, 1, 1), n)) as sm:
                    block["calls"] += measure("%d --simplify %d" % (r, n), sm)
            if args.full:
                block["calls"] += measure("%d" % r, cm)
        results.append(block)

    res = dict(metric="mesh_project_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), views=len(views), image=args.res, format="uint16", repeat=args.repeat, results=results,
               defaults_table=table)
    common.report(res, args.out)
    c.close()


if __name__ == "__main__":
    main()
