#!/usr/bin/env python3
"""Cost and findings of the self-intersection stage on one MI355X: rnb_mesh_intersections and rnb_mesh_intersections_select (include/rnb_mesh_intersect.h) beside the
topology stage's census on the same mesh.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_clean.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh, colours) and measured in three forms:
  raw        the extraction as it comes
  simplified after DeviceMesh.simplify on --simplify cells per axis over the unit cube (one vertex per cell: a sheet can be pulled through its neighbour)
  filled     what the scene's views see, triangle by triangle (DeviceMesh.cull_unseen(views, unit="faces")), with a seeded --punch fraction of its triangles removed
             (default 1 %, as tools/bench_mesh_holes.py), after DeviceMesh.fill_holes(): fans over rims that were never planar
On each, over --rounds rounds with the first untimed (median and min .. max of stats.ms):
  census     DeviceMesh.self_intersections(): the counts per triangle and the statistics (downloads not in stats.ms)
  topology   DeviceMesh.topology() on the same mesh: an accepted stage as the yardstick
and once: the census with the pair list; DeviceMesh.drop_intersecting() followed by fill_holes(), and the census of what that leaves. No time is a pass criterion.

  python tools/bench_mesh_intersections.py [--steps 2000] [--resolution 512 1024] [--rounds 5] [--simplify 128] [--punch 0.01] [--out profiles/mesh_intersections.json]
                                           [--markdown profiles/mesh_intersections.md]

Prints one JSON line (and writes it to --out when given; the table to --markdown when given).
"""
import json
import os
import subprocess
import sys

import numpy as np

import mesh_bench_common as common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUND = ("n_degenerate", "n_same_set", "n_candidates", "n_pairs_proper", "n_pairs_contact", "n_tris_proper", "n_tris_contact", "n_coplanar_pairs")
GRID = ("dims", "n_large", "n_cell_entries", "n_visited", "peak_workspace")


def measure(m, rounds):
    """One device mesh: the census and the topology stage over `rounds` rounds; the pair list, the drop and the fill once."""
    row = dict(n_verts=m.n_verts, n_triangles=m.n_triangles)
    runs = [m.self_intersections() for _ in range(rounds)]
    last = runs[-1]
    row["census"] = dict(common.spread([r["ms"] for r in runs], "ms_"), **common.spread([r["ms_grid"] for r in runs], "ms_grid_"), **{k: last[k] for k in FOUND + GRID})
    row["candidates_per_triangle"] = round(last["n_candidates"] / max(m.n_triangles, 1), 3)
    row["visited_per_candidate"] = round(last["n_visited"] / max(last["n_candidates"], 1), 3)
    row["ms_with_pairs"] = round(m.self_intersections(pairs=True)["ms"], 3)
    runs = [m.topology() for _ in range(rounds)]
    row["topology"] = dict(common.spread([r["ms"] for r in runs], "ms_"), closed=runs[-1]["closed"], n_boundary_edges=runs[-1]["n_boundary_edges"])
    with m.drop_intersecting() as dropped, dropped.fill_holes() as filled:
        after = filled.self_intersections()
        row["drop"] = {k: v for k, v in dropped.stats.items() if k != "census"}
        row["refill"] = {k: filled.stats[k] for k in ("n_loops", "n_filled", "n_skipped_not_simple", "n_tris_added", "ms")}
        row["after_drop_and_fill"] = dict({k: after[k] for k in FOUND}, closed=filled.topology()["closed"])
    return row


def kernel_resources():
    """The lines of tools/kernel_resources.sh for the stage's kernels, or why there are none."""
    try:
        r = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), "k_mi_"], capture_output=True, text=True, timeout=300)
        return r.stdout.strip().splitlines() or [r.stderr.strip() or "no output"]
    except (OSError, subprocess.TimeoutExpired) as e:
        return ["not available: %s" % e]


def markdown(res):
    lines = ["# Mesh self-intersections: census, drop and refill on the MI355X", "",
             "Measured by `tools/bench_mesh_intersections.py` (%d training steps, %d rounds, the first untimed; medians of `stats.ms`, min .. max in the JSON beside this file)." % (
                 res["train_steps"], res["rounds"]),
             "`census` = `DeviceMesh.self_intersections()`, `topology` = `DeviceMesh.topology()` on the same mesh (the yardstick of an accepted stage), `with pairs` = the census",
             "with the sorted pair list, once.", "",
             "Measured: the wall-clock time of each call as the library reports it (`stats.ms`: allocation, the index check, the grid, the pair kernels and the device-to-host reads",
             "of the counts), of which `grid` is the box and the cell lists; the candidates per triangle; the pairs the search looked at per candidate (what the grid costs in box",
             "tests). Not measured: how the pair kernel's time divides between the gathers, the staging and the sign arithmetic (no counter was read), nor its occupancy at run time.", "",
             "| mesh | triangles | census ms | grid ms | with pairs ms | topology ms | candidates / triangle | visited / candidate | grid | cell entries | peak workspace MB |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        s = r["census"]
        lines.append("| %s | %d | %.3f | %.3f | %.3f | %.3f | %.2f | %.2f | %s | %d | %.1f |" % (
            r["mesh"], r["n_triangles"], s["ms_median"], s["ms_grid_median"], r["ms_with_pairs"], r["topology"]["ms_median"], r["candidates_per_triangle"], r["visited_per_candidate"],
            "x".join(str(d) for d in s["dims"]), s["n_cell_entries"], s["peak_workspace"] / 1e6))
    lines += ["", "## What the census finds, and what `drop_intersecting()` + `fill_holes()` leave", "",
              "| mesh | proper pairs | contact pairs | triangles proper / contact | coplanar pairs | degenerate | dropped triangles | loops refilled | proper / contact pairs after | closed before -> after |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        s, a = r["census"], r["after_drop_and_fill"]
        lines.append("| %s | %d | %d | %d / %d | %d | %d | %d | %d of %d | %d / %d | %d -> %d |" % (
            r["mesh"], s["n_pairs_proper"], s["n_pairs_contact"], s["n_tris_proper"], s["n_tris_contact"], s["n_coplanar_pairs"], s["n_degenerate"], r["drop"]["n_tris_removed"],
            r["refill"]["n_filled"], r["refill"]["n_loops"], a["n_pairs_proper"], a["n_pairs_contact"], r["topology"]["closed"], a["closed"]))
    lines += ["", "## Kernel resources (`tools/kernel_resources.sh k_mi_`)", "", "```"] + res["kernel_resources"] + ["```", "",
              "The pair kernels use no scratch. With the sign routines as real functions they did: 1088 bytes per lane with every routine a call, 448 with `mi_orient` alone (the calls",
              "keep their live registers there), so every routine is inlined; the price is 141 VGPRs, three wavefronts per SIMD."]
    return "\n".join(lines) + "\n"


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--simplify", type=int, default=128)
    ap.add_argument("--punch", type=float, default=0.01)
    ap.add_argument("--markdown", default=None)
    args = common.parse_args(ap)

    c, scene, train_s = common.train_scene(args)
    views = scene[0]
    results = []

    def add(name, r, m):
        row = dict(mesh="%d^3 extraction, %s" % (r, name), resolution=r, **measure(m, args.rounds))
        results.append(row)
        print(json.dumps(row), file=sys.stderr)

    for r in args.resolution:
        with c.extract_mesh_device(r, colors=True) as m:
            add("raw", r, m)
            with m.simplify((0.0, 0.0, 0.0), 1.0 / args.simplify, args.simplify) as sm:
                add("simplified on %d^3 cells" % args.simplify, r, sm)
            with m.cull_unseen(views, unit="faces") as seen:
                d = seen.download()
            tris = d["indices"].reshape(-1, 3)
            keep = np.random.default_rng(r).random(len(tris)) >= args.punch
            with c.upload_mesh(d["verts"], tris[keep].ravel(), d.get("colors")) as punched, punched.fill_holes() as filled:
                add("seen faces, %g %% of the triangles removed, holes filled" % (100 * args.punch), r, filled)

    res = dict(metric="mesh_intersections_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, punch=args.punch, simplify=args.simplify,
               results=results, kernel_resources=kernel_resources())
    common.report(res, args.out)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(res))
    c.close()


if __name__ == "__main__":
    main()
