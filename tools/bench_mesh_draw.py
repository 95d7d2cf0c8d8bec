#!/usr/bin/env python3
"""Cost of rnb_mesh_draw_textured (include/rnb_mesh_draw.h) on one MI355X beside rnb_mesh_raster of the same mesh and view, and the per-view numbers the draw exists for.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_raster.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh) and cleaned (rnb_mesh_clean, largest, outward) once, and simplified (quadric placement) on N^3 cells for every N of --cells; the
cleaned mesh itself is measured too (--no-full leaves it out). Every one of these device meshes gets the model's bake (albedo + normal) at --size S -- or, where the atlas
of S does not hold the mesh, at the smallest power of two up to 8192 that does -- and is drawn into the first --draw-views views (the cleaned meshes, whose maps of 0.25 to
1 GiB each the interface uploads with every call: into the first --full-draw-views), the image left on the device (out_ptr): ms per view (stats.ms, the median over the views of the per-view median of --repeat calls after one untimed call) of
  raster            rnb_mesh_raster: the baseline, code this stage does not touch
  draw_one_map      the colour map alone, bilinear
  draw_two_maps     colour and normal map, bilinear
  draw_nearest      colour and normal map, nearest
`extra_ms` = draw_two_maps - raster is what the texture-sampling resolve costs beyond the plain one; `gather_gb_s` is that difference against its gather traffic, computed
here from the counts: covered pixels x (4 taps x 16 B x 2 maps + 24 B of uv); it is left out (null) where the difference is not above the spread of the raster's own times over
the views (max - min): the times are those of whole calls, which allocate, clear and synchronise (a kernel trace then tells the two resolves apart: profiles/mesh_draw.md). The condition of the stage is
extra_ms < raster ms (`extra_below_raster`).

The numbers the stage exists for, per mesh over all views (Context.mesh_view_metrics): the mean normal angle of the bare mesh and of the normal-mapped one, and the
albedo PSNR against the input albedo maps of the model's bake and of the texture project_views blends from those maps.

  python tools/bench_mesh_draw.py [--steps 2000] [--resolution 512 1024] [--cells 128] [--no-full] [--size 2048] [--repeat 3] [--draw-views 64] [--full-draw-views 8]
                                  [--out profiles/mesh_draw.json]

Prints one JSON line (and writes it to --out when given, with a table of it beside it as <out without its suffix>.table.md; profiles/mesh_draw.md is that table and its reading, written by hand).
"""
import json
import os
import sys

import numpy as np

import mesh_bench_common as common

CHANNELS = 9


def fin(x, digits):
    """A rounded number for the JSON line; "inf" for what is not finite (a PSNR of identical images)."""
    return round(float(x), digits) if np.isfinite(x) else "inf"


def table(res):
    """The markdown table of a result."""
    lines = ["| mesh | triangles | S | raster ms | draw, one map | draw, two maps | nearest | extra ms | gather GB/s | angle bare | angle mapped | PSNR bake | PSNR projected |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for block in res["results"]:
        for r in block["calls"]:
            if "skipped" in r:
                lines.append("| %s | %d | | skipped: %s | | | | | | | | | |" % (r["mesh"], r["n_tris"], r["skipped"]))
                continue
            lines.append("| %s | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %s | %.3f | %.3f | %s | %s |" % (
                r["mesh"], r["n_tris"], r["size"], r["raster_ms"]["median"], r["draw_one_map_ms"]["median"], r["draw_two_maps_ms"]["median"], r["draw_nearest_ms"]["median"], r["extra_ms"],
                "within the spread" if r["gather_gb_s"] is None else r["gather_gb_s"], r["angle_bare_deg"], r["angle_mapped_deg"], r["psnr_bake_db"], r["psnr_projected_db"]))
    return "\n".join(lines) + "\n"


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--cells", type=int, nargs="*", default=[128], help="N of the simplifications")
    ap.add_argument("--no-full", dest="full", action="store_false", help="leave out the cleaned mesh without simplification")
    ap.add_argument("--full-draw-views", type=int, default=8, help="the views the times of the cleaned meshes are taken in")
    ap.add_argument("--size", type=int, default=2048, help="texels per side")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--draw-views", type=int, default=64, help="the views the times are taken in (the metrics use all of them)")
    args = common.parse_args(ap)

    c, (views, normals, albedos), train_s = common.train_scene(args)
    images = [np.asarray(a).reshape(v["height"], v["width"], 4) for v, a in zip(views, albedos)]
    from rnb_neus2_amd import api
    out_ptr = c.device_malloc(max(v["width"] * v["height"] for v in views) * CHANNELS * 4)

    def per_view(call, timed):
        """Median over the timed views of the per-view median ms; the covered pixels of the last call per view, summed."""
        meds, covered = [], 0
        for view in timed:
            runs = [call(view) for _ in range(args.repeat + 1)]
            meds.append(float(np.median([r["ms"] for r in runs[1:]])))
            covered += runs[-1]["n_covered"]
        return common.spread(meds, untimed=0), covered

    def measure(name, m, n_timed):
        timed, size = views[:max(1, n_timed)], args.size
        while True:  # the smallest power of two from --size up whose atlas holds the mesh
            try:
                api.Context.texture_layout(m.n_triangles, size)
                break
            except (api.RnbError, ValueError) as e:
                if size >= 8192:
                    row = dict(mesh=name, n_tris=m.n_triangles, skipped=str(e)[-120:])
                    print(json.dumps(row), file=sys.stderr)
                    return [row]
                size *= 2
        baked = m.bake_texture(size, maps=("albedo", "normal"))
        uv, albedo, normal = baked["uv"], baked["albedo"], baked["normal"]
        raster, covered = per_view(lambda v: m.rasterize(v, out_ptr=out_ptr), timed)
        one, _ = per_view(lambda v: m.draw_textured(v, uv, albedo, out_ptr=out_ptr), timed)
        two, _ = per_view(lambda v: m.draw_textured(v, uv, albedo, normal, out_ptr=out_ptr), timed)
        near, _ = per_view(lambda v: m.draw_textured(v, uv, albedo, normal, filter="nearest", out_ptr=out_ptr), timed)
        extra = two["median"] - raster["median"]
        gather = covered / len(timed) * (4 * 16 * 2 + 24)  # bytes per view
        mesh = m.download()
        tris = mesh["indices"].reshape(-1, 3)
        bare = c.mesh_view_metrics(mesh["verts"], tris, views, normals)
        mapped = c.mesh_view_metrics(mesh["verts"], tris, views, normals, texture=dict(uv=uv, color=albedo, normal=normal), albedo_maps=images)
        proj = m.project_views(views, images, size=size, fallback="model")
        projected = c.mesh_view_metrics(mesh["verts"], tris, views, normals, texture=dict(uv=proj["uv"], color=proj["color"]), albedo_maps=images)
        row = dict(mesh=name, n_tris=m.n_triangles, size=size, timed_views=len(timed), covered_per_view=round(covered / len(timed)), raster_ms=raster, draw_one_map_ms=one, draw_two_maps_ms=two, draw_nearest_ms=near,
                   extra_ms=round(extra, 3), extra_below_raster=bool(extra < raster["median"]), gather_gb_s=round(gather / extra / 1e6, 1) if extra > raster["max"] - raster["min"] else None,
                   angle_bare_deg=round(bare["mean"]["mean_angle_deg"], 4), angle_mapped_deg=round(mapped["mean"]["mean_angle_deg"], 4),
                   psnr_bake_db=fin(mapped["mean"]["albedo_psnr_db"], 3), psnr_projected_db=fin(projected["mean"]["albedo_psnr_db"], 3),
                   mae_bake=round(mapped["mean"]["albedo_mae"], 5), mae_projected=round(projected["mean"]["albedo_mae"], 5))
        print(json.dumps(row), file=sys.stderr)
        return [row]

    results = []
    for r in args.resolution:
        with c.extract_mesh_device(r) as m:
            cm = m.clean("largest", "outward")
        with cm:
            block = dict(resolution=r, calls=[])
            for n in args.cells:
                with cm.simplify(*c.simplify_grid((0, 0, 0), (1, 1, 1), n)) as sm:
                    block["calls"] += measure("%d --simplify %d" % (r, n), sm, args.draw_views)
            if args.full:
                block["calls"] += measure("%d" % r, cm, args.full_draw_views)
        results.append(block)
    c.device_free(out_ptr)

    res = dict(metric="mesh_draw_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), views=len(views), image=args.res, size=args.size, repeat=args.repeat,
               results=results)
    common.report(res, args.out)
    if args.out:
        with open(os.path.splitext(args.out)[0] + ".table.md", "w") as f:
            f.write(table(res))
    c.close()


if __name__ == "__main__":
    main()
