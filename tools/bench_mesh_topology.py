#!/usr/bin/env python3
"""Cost of the topology stage on one MI355X: rnb_mesh_topology and rnb_mesh_repair (include/rnb_mesh_topology.h) beside the cleaner and the host stage they replace.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_clean.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh, colours) and simplified on (R / 4)^3 cells over the unit box (rnb_mesh_simplify, quadric placement), and on both meshes, over
--rounds rounds with the first untimed (median and min .. max of stats.ms):
  topology   DeviceMesh.topology(edges=True, table=True): the census with the three per-half-edge arrays and the component table (downloads not in stats.ms)
  repair     DeviceMesh.repair(duplicates="cancel", orient="consistent")
  clean      DeviceMesh.clean("largest", "outward") on the same mesh: a stage of like traffic (components, sums, compaction)
and once, on a downloaded copy, meshproc.Mesh.fix_normals, the host stage the repair's orient step replaces. The meshes are visited in ascending size; once the host
stage has taken more than --host-limit-s seconds (default 60) it is skipped for the larger ones and reported as such. The census of every mesh is printed with its times.

  python tools/bench_mesh_topology.py [--steps 2000] [--resolution 512 1024] [--rounds 5] [--host-limit-s 60] [--out profiles/mesh_topology.json] [--markdown profiles/mesh_topology.md]

Prints one JSON line (and writes it to --out when given; the table to --markdown when given).
"""
import json
import sys
import time

import mesh_bench_common as common

CENSUS = ("n_verts_used", "n_tris", "n_degenerate", "n_edges", "n_boundary_edges", "n_manifold_edges", "n_nonmanifold_edges", "n_inconsistent_edges", "max_faces_on_edge",
          "n_duplicate_tris", "n_folded_pairs", "n_components", "n_patches", "n_unorientable_patches", "n_boundary_components", "closed", "oriented", "euler")


def measure(m, rounds, host, meshproc):
    """One device mesh: the three device stages over `rounds` rounds, the host stage once when `host`."""
    row = dict(n_verts=m.n_verts, n_triangles=m.n_triangles)
    runs = [m.topology(edges=True, table=True) for _ in range(rounds)]
    row["census"] = {k: runs[-1][k] for k in CENSUS}
    row["genus"] = [int(g) for g in runs[-1]["table"]["genus"][:8]]
    row["topology"] = dict(common.spread([r["ms"] for r in runs], "ms_"), peak_workspace=runs[-1]["peak_workspace"])
    stats = []
    for _ in range(rounds):
        with m.repair(duplicates="cancel", orient="consistent") as r:
            stats.append(r.stats)
    row["repair"] = dict(common.spread([s["ms"] for s in stats], "ms_"), **{k: v for k, v in stats[-1].items() if k != "ms"})
    stats = []
    for _ in range(rounds):
        with m.clean("largest", "outward") as r:
            stats.append(r.stats)
    row["clean"] = dict(common.spread([s["ms"] for s in stats], "ms_"), n_components=stats[-1]["n_components"], n_tris_out=stats[-1]["n_tris_out"])
    if host:
        d = m.download()
        mesh = meshproc.Mesh(d["verts"], d["indices"].reshape(-1, 3).astype("int64"))
        t = time.perf_counter()
        mesh.fix_normals()
        row["host_fix_normals_s"] = round(time.perf_counter() - t, 3)
        row["repair_speedup_over_host"] = round(row["host_fix_normals_s"] * 1e3 / row["repair"]["ms_median"], 1)
    else:
        row["host_fix_normals_s"] = None
    return row


def markdown(res):
    lines = ["# Mesh topology: census and repair on the MI355X", "",
             "Measured by `tools/bench_mesh_topology.py` (%d training steps, %d rounds, the first untimed; medians of `stats.ms`, min .. max in the JSON beside this file)." % (
                 res["train_steps"], res["rounds"]),
             "`topology` = `DeviceMesh.topology(edges=True, table=True)`, `repair` = `DeviceMesh.repair(duplicates=\"cancel\", orient=\"consistent\")`, `clean` = `rnb_mesh_clean`",
             "(largest, outward) on the same mesh, `host` = `meshproc.Mesh.fix_normals` on a downloaded copy, once.", "",
             "| mesh | triangles | topology ms | repair ms | clean ms | host fix_normals s | repair vs host |", "|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        host = "skipped (over the limit)" if r["host_fix_normals_s"] is None else "%.3f" % r["host_fix_normals_s"]
        speed = "" if r["host_fix_normals_s"] is None else "%.0f x" % r["repair_speedup_over_host"]
        lines.append("| %s | %d | %.3f | %.3f | %.3f | %s | %s |" % (r["mesh"], r["n_triangles"], r["topology"]["ms_median"], r["repair"]["ms_median"], r["clean"]["ms_median"], host, speed))
    lines += ["", "## Census", "", "| mesh | " + " | ".join(CENSUS) + " | genus (first components) |", "|---|" + "---|" * (len(CENSUS) + 1)]
    for r in res["results"]:
        lines.append("| %s | " % r["mesh"] + " | ".join(str(r["census"][k]) for k in CENSUS) + " | %s |" % r["genus"])
    lines += ["", "## Repair", "", "| mesh | duplicates dropped | degenerate dropped | flipped | patches | unorientable | triangles out | peak workspace MB |", "|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        s = r["repair"]
        lines.append("| %s | %d | %d | %d | %d | %d | %d | %.1f |" % (r["mesh"], s["n_duplicates_dropped"], s["n_degenerate_dropped"], s["n_flipped"], s["n_patches"], s["n_unorientable_patches"],
                                                               s["n_tris_out"], s["peak_workspace"] / 1e6))
    return "\n".join(lines) + "\n"


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-limit-s", type=float, default=60.0)
    ap.add_argument("--markdown", default=None)
    args = common.parse_args(ap)

    from rnb_neus2_amd import meshproc

    c, _, train_s = common.train_scene(args)
    todo = []  # (name, resolution, cells or None)
    for r in args.resolution:
        todo += [("%d^3 extraction" % r, r, None), ("%d^3 simplified on %d^3 cells" % (r, r // 4), r, r // 4)]
    results, host = [], True
    pending = []
    for name, r, cells in todo:  # sizes first, so that the host stage meets the meshes in ascending size
        with c.extract_mesh_device(r, colors=True) as m:
            if cells is None:
                pending.append((m.n_triangles, name, r, cells))
            else:
                with m.simplify(*c.simplify_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), cells)) as sm:
                    pending.append((sm.n_triangles, name, r, cells))
    for _, name, r, cells in sorted(pending):
        with c.extract_mesh_device(r, colors=True) as m:
            if cells is None:
                row = measure(m, args.rounds, host, meshproc)
            else:
                with m.simplify(*c.simplify_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), cells)) as sm:
                    row = measure(sm, args.rounds, host, meshproc)
        row = dict(mesh=name, resolution=r, cells=cells, **row)
        if row["host_fix_normals_s"] is not None and row["host_fix_normals_s"] > args.host_limit_s:
            host = False
        results.append(row)
        print(json.dumps(row), file=sys.stderr)

    res = dict(metric="mesh_topology_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, host_limit_s=args.host_limit_s, results=results)
    common.report(res, args.out)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(res))
    c.close()


if __name__ == "__main__":
    main()
