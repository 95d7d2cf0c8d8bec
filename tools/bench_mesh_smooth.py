#!/usr/bin/env python3
"""Cost and effect of the smoothing stage on one MI355X: rnb_mesh_smooth and rnb_mesh_vertex_normals (include/rnb_mesh_smooth.h) beside the topology stage's census and
the numpy statement of tests/mesh_smooth_reference.py, and the quality table behind the default number of passes.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_clean.py). Then at each --resolution R
three meshes are measured: the extraction (rnb_extract_mesh, colours), its --simplify N version (vertex clustering, repaired), and that one after drop + fill
(DeviceMesh.drop_intersecting, DeviceMesh.fill_holes). On each, over --rounds rounds with the first untimed (median and min .. max of stats.ms):
  smooth     DeviceMesh.smooth(passes=--passes): ms per call, ms per pass (stats.ms_passes / passes), the bytes the loads and stores of a pass ask for (per moving
             vertex its position read and written, per neighbour-list entry its index and the neighbour's position, gathered once per entry: most of those hit in
             cache) and the rate that makes of ms per pass, against the bytes of the mesh itself; how many vertices take the wide path
  normals    DeviceMesh.vertex_normals()
  topology   DeviceMesh.topology() on the same mesh: the stage whose edge join the smoothing runs first
and once, on a downloaded copy, the numpy reference (expected_smooth) where the mesh has at most --reference-limit vertices, and whether the device equals it bit for bit.
The quality table, for passes 0, 2, 5, 10, 20, 50 on every mesh (measured against the scene's views at --quality-views of them): Context.mesh_view_metrics' mean normal
angle and mask IoU against the input normal maps, DeviceMesh.distance_to the unsmoothed mesh (mean, max), and the proper self-intersections after smoothing
(DeviceMesh.self_intersections). No time is a pass criterion.

  python tools/bench_mesh_smooth.py [--steps 2000] [--resolution 512 1024] [--simplify 128] [--rounds 5] [--passes 10] [--out profiles/mesh_smooth.json] [--markdown profiles/mesh_smooth.md]

Prints one JSON line (and writes it to --out when given; the tables to --markdown when given).
"""
import json
import sys
import time

import mesh_bench_common as common

PASSES = (0, 2, 5, 10, 20, 50)


def measure(c, m, rounds, reference_limit, passes):
    """One device mesh: the three device stages over `rounds` rounds, the numpy reference once."""
    from tests import mesh_smooth_reference as sr
    row = dict(n_verts=m.n_verts, n_triangles=m.n_triangles, mesh_bytes=m.n_verts * 12 + m.n_indices * 4)
    stats = []
    for _ in range(rounds):
        with m.smooth(passes=passes) as s:
            stats.append(s.stats)
    last = stats[-1]
    per_pass = [s["ms_passes"] / max(s["passes"], 1) for s in stats]
    with m.smooth(passes=0, census=True) as census:  # the neighbour lists' entries: the valences of the moving vertices (the interior ones: the boundary is pinned)
        entries = int(census.valence[census.kind == 1].sum())
    row["smooth"] = dict(common.spread([s["ms"] for s in stats], "ms_"), **common.spread(per_pass, "ms_per_pass_", digits=4), **{k: v for k, v in last.items() if k not in ("ms", "ms_passes")})
    # what a pass asks for: 48 bytes per moving vertex (P read, P written), 28 per list entry (index, the neighbour's P); entries: the sum of m over the moving vertices
    row["pass_bytes"] = 48 * last["n_moving"] + 28 * entries
    row["pass_gb_s"] = round(row["pass_bytes"] / (row["smooth"]["ms_per_pass_median"] * 1e-3) / 1e9, 1) if row["smooth"]["ms_per_pass_median"] > 0 else None
    runs = [m.vertex_normals() for _ in range(rounds)]
    row["normals"] = dict(common.spread([r["ms"] for r in runs], "ms_"), n_zero=runs[-1]["n_zero"], max_corners=runs[-1]["max_corners"])
    runs = [m.topology() for _ in range(rounds)]
    row["topology"] = dict(common.spread([r["ms"] for r in runs], "ms_"), n_edges=runs[-1]["n_edges"], n_boundary_edges=runs[-1]["n_boundary_edges"])
    if m.n_verts <= reference_limit:
        d = m.download()
        t = time.perf_counter()
        want = sr.expected_smooth(d["verts"], d["indices"], passes=passes)
        row["reference_s"] = round(time.perf_counter() - t, 3)
        with m.smooth(passes=passes) as s:
            got = s.download()
        row["equal_bits"] = bool(got["verts"].tobytes() == want["verts"].tobytes())
    else:
        row["reference_s"] = row["equal_bits"] = None
    return row


def quality(c, m, views, normal_maps):
    """The table behind the default: per number of passes the view metrics, the distance to the unsmoothed mesh and the proper self-intersections."""
    rows = []
    for passes in PASSES:
        with m.smooth(passes=passes) as s:
            d = s.download()
            met = c.mesh_view_metrics(d["verts"], d["indices"], views, normal_maps)["mean"]
            dist = s.distance_to(m)
            si = s.self_intersections()
            rows.append(dict(passes=passes, mean_angle_deg=met["mean_angle_deg"], median_angle_deg=met["median_angle_deg"], mask_iou=met["mask_iou"], distance_mean=dist["mean"],
                             distance_max=dist["max"], n_pairs_proper=si["n_pairs_proper"], n_tris_proper=si["n_tris_proper"], max_displacement=s.stats["max_displacement"]))
    return rows


def markdown(res):
    lines = ["# Mesh smoothing: Taubin passes over the one-ring and ring normals on the MI355X", "",
             "Measured by `tools/bench_mesh_smooth.py` (%d training steps, %d rounds, the first untimed; medians of `stats.ms`, min .. max in the JSON beside this file)." % (
                 res["train_steps"], res["rounds"]),
             "`smooth` = `DeviceMesh.smooth(passes=%d)`, `per pass` = `stats.ms_passes / passes`, `normals` = `DeviceMesh.vertex_normals()`," % res["timed_passes"],
             "`topology` = `DeviceMesh.topology()` on the same mesh, `reference` = `tests/mesh_smooth_reference.expected_smooth` on a downloaded copy, once, and whether the",
             "device's vertices equal it bit for bit.", "",
             "Measured: the wall-clock time of each call as the library reports it (allocation, the edge join and the device-to-host reads of the counts included), the time of",
             "the passes alone (between two synchronisations), the peak workspace. `pass GB/s` divides the bytes the loads and stores of a pass ask for (48 per moving vertex, 28 per neighbour-list",
             "entry: a neighbour's position is gathered once per entry, and most of those loads hit in cache, which is how the figure can pass the memory's own rate) by the time per",
             "pass; `x mesh` is that byte count over the mesh's own size (12 bytes per vertex, 4 per index). Not measured: how the rest of a call divides",
             "between the edge join, the list fill and the copies (no kernel was timed on its own), and the hardware's own byte counters.", "",
             "| mesh | vertices | triangles | smooth ms | per pass ms | pass GB/s | x mesh | wide vertices | max valence | normals ms | topology ms | reference s | equal bits | peak workspace MB |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        ref = "not run (over the limit)" if r["reference_s"] is None else "%.3f" % r["reference_s"]
        s = r["smooth"]
        lines.append("| %s | %d | %d | %.3f | %.4f | %s | %.2f | %d | %d | %.3f | %.3f | %s | %s | %.1f |" % (
            r["mesh"], r["n_verts"], r["n_triangles"], s["ms_median"], s["ms_per_pass_median"], r["pass_gb_s"], r["pass_bytes"] / max(r["mesh_bytes"], 1), s["n_wide"], s["max_valence"],
            r["normals"]["ms_median"], r["topology"]["ms_median"], ref, r["equal_bits"], s["peak_workspace"] / 1e6))
    lines += ["", "## Quality by number of passes", "",
              "lambda 0.5, mu -0.53, boundary pinned. Normal angle and mask IoU: `Context.mesh_view_metrics` against the input normal maps of %d views, the means over the views;" % res["quality_views"],
              "distance: `DeviceMesh.distance_to` the unsmoothed mesh; proper pairs: `DeviceMesh.self_intersections` of the smoothed mesh. The row of 0 passes is the unsmoothed mesh.",
              "The default number of passes has to be a row that lowers the mean normal angle against the row of 0 passes and adds no proper pair.", "",
              "| mesh | passes | mean angle deg | median angle deg | mask IoU | distance mean | distance max | proper pairs | max displacement |", "|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        for q in r["quality"]:
            lines.append("| %s | %d | %.4f | %.4f | %.5f | %.3g | %.3g | %d | %.3g |" % (r["mesh"], q["passes"], q["mean_angle_deg"], q["median_angle_deg"], q["mask_iou"], q["distance_mean"],
                                                                                 q["distance_max"], q["n_pairs_proper"], q["max_displacement"]))
    lines += ["", "## The default", "",
              "The default was Taubin's customary ten passes until this table was first made. On the extracted meshes every row lowers the mean angle, and more passes lower it",
              "further; on the clustered meshes only one pair does: from five passes on the mean angle rises above the unsmoothed mesh's (at five and ten passes the median",
              "still falls), and some rows add a proper self-intersection. The default is therefore the row that holds on every mesh; ask for more passes on an",
              "extraction that is not simplified.", ""] + res["default_verdict"]
    return "\n".join(lines) + "\n"


def verdict(results, default_passes):
    """What the quality table says about the default, in words, from the rows themselves."""
    out = []
    for r in results:
        base = r["quality"][0]
        ok = [q["passes"] for q in r["quality"][1:] if q["mean_angle_deg"] < base["mean_angle_deg"] and q["n_pairs_proper"] <= base["n_pairs_proper"]]
        out.append("* %s: the rows that lower the mean normal angle and add no proper self-intersection: %s." % (r["mesh"], ", ".join(str(p) for p in ok) if ok else "none"))
    every = all(default_passes in [q["passes"] for q in r["quality"][1:] if q["mean_angle_deg"] < r["quality"][0]["mean_angle_deg"] and q["n_pairs_proper"] <= r["quality"][0]["n_pairs_proper"]]
                for r in results)
    out.append("")
    out.append("The default of %d passes %s on every mesh measured here. `Context.extract_mesh` and `build/mesh` smooth only when asked to." % (
        default_passes, "is such a row" if every else "is NOT such a row"))
    return out


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--simplify", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=10, help="the passes of the timed calls")
    ap.add_argument("--reference-limit", type=int, default=1500000)
    ap.add_argument("--quality-views", type=int, default=8)
    ap.add_argument("--markdown", default=None)
    args = common.parse_args(ap)

    c, scene, train_s = common.train_scene(args)
    step = max(len(scene[0]) // max(args.quality_views, 1), 1)
    views, normal_maps = scene[0][::step][:args.quality_views], scene[1][::step][:args.quality_views]
    results = []

    def one(name, r, m):
        row = dict(mesh=name, resolution=r, **measure(c, m, args.rounds, args.reference_limit, args.passes))
        row["quality"] = quality(c, m, views, normal_maps)
        results.append(row)
        print(json.dumps(row), file=sys.stderr)

    grid = c.simplify_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), args.simplify)
    for r in args.resolution:
        with c.extract_mesh_device(r, colors=True) as m:
            one("%d^3 extraction" % r, r, m)
            with m.simplify(*grid) as sm, sm.repair() as rm:
                one("%d^3, simplify %d" % (r, args.simplify), r, rm)
                with rm.drop_intersecting() as dm, dm.fill_holes() as fm:
                    one("%d^3, simplify %d, drop + fill" % (r, args.simplify), r, fm)

    with c.upload_mesh([[0.0, 0.0, 0.0]], []) as point, point.smooth() as s:  # what the library calls its default
        default_passes = s.stats["passes"]
    res = dict(metric="mesh_smooth_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, timed_passes=args.passes, default_passes=default_passes, quality_views=len(views),
               results=results, default_verdict=verdict(results, default_passes))
    common.report(res, args.out)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(res))
    c.close()


if __name__ == "__main__":
    main()
