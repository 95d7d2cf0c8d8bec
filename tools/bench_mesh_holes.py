#!/usr/bin/env python3
"""Cost of the hole stage on one MI355X: rnb_mesh_boundary_loops and rnb_mesh_fill_holes (include/rnb_mesh_holes.h) beside the topology stage's census and the numpy
statement of tests/mesh_holes_reference.py.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_clean.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh, colours) and loses what none of the scene's views sees, triangle by triangle (DeviceMesh.cull_unseen(views, unit="faces"): the
stage that makes holes on purpose); a second mesh is the same one with a seeded --punch fraction of its triangles removed (default 1 %). On both, over --rounds rounds
with the first untimed (median and min .. max of stats.ms):
  loops      DeviceMesh.boundary_loops(edges=True, table=True): the census with the three per-half-edge arrays and the loop table (downloads not in stats.ms)
  fill       DeviceMesh.fill_holes()
  topology   DeviceMesh.topology() on the same mesh: the stage whose edge join the hole stage runs first
and once, on a downloaded copy, the numpy reference (expected_fill) where the mesh has at most --reference-limit boundary edges. The loops of every mesh are reported by
size, and closed / oriented of DeviceMesh.topology() after the fill. No time is a pass criterion.

  python tools/bench_mesh_holes.py [--steps 2000] [--resolution 512 1024] [--rounds 5] [--punch 0.01] [--out profiles/mesh_holes.json] [--markdown profiles/mesh_holes.md]

Prints one JSON line (and writes it to --out when given; the table to --markdown when given).
"""
import json
import sys
import time

import numpy as np

import mesh_bench_common as common

SIZES = ((3, 3), (4, 4), (5, 8), (9, 64), (65, 1024), (1025, 1 << 20))  # loop sizes reported together, in edges


def measure(c, m, rounds, reference_limit):
    """One device mesh: the three device stages over `rounds` rounds, the numpy reference once."""
    from tests import mesh_holes_reference as hr
    row = dict(n_verts=m.n_verts, n_triangles=m.n_triangles)
    runs = [m.boundary_loops(edges=True, table=True) for _ in range(rounds)]
    last = runs[-1]
    row["loops"] = dict(common.spread([r["ms"] for r in runs], "ms_"), **{k: last[k] for k in hr.LOOPS_STATS}, peak_workspace=last["peak_workspace"])
    n = last["table"]["n_edges"]
    row["loop_sizes"] = {("%d" % lo if lo == hi else "%d-%d" % (lo, hi)): int(((n >= lo) & (n <= hi)).sum()) for lo, hi in SIZES}
    row["ranking_rounds"] = int(np.ceil(np.log2(max(int(n[last["table"]["simple"] == 1].max()) if last["n_simple"] else 1, 1))))
    stats = []
    for _ in range(rounds):
        with m.fill_holes() as f:
            stats.append(f.stats)
            after = f.topology()
    row["fill"] = dict(common.spread([s["ms"] for s in stats], "ms_"), **{k: v for k, v in stats[-1].items() if k != "ms"})
    row["after_fill"] = {k: after[k] for k in ("closed", "oriented", "n_boundary_edges", "n_boundary_components", "n_nonmanifold_edges", "euler")}
    runs = [m.topology() for _ in range(rounds)]
    row["topology"] = dict(common.spread([r["ms"] for r in runs], "ms_"), n_boundary_components=runs[-1]["n_boundary_components"], euler=runs[-1]["euler"])
    if last["n_boundary_edges"] <= reference_limit:
        d = m.download()
        t = time.perf_counter()
        want = hr.expected_fill(d["verts"], d["indices"], d.get("colors"))
        row["reference_s"] = round(time.perf_counter() - t, 3)
        with m.fill_holes() as f:
            got = f.download()
        row["equal_bits"] = bool(all(got[k].tobytes() == want[k].tobytes() for k in ("verts", "indices", "colors") if k in got))
    else:
        row["reference_s"] = row["equal_bits"] = None
    return row


def markdown(res):
    lines = ["# Mesh holes: boundary loops and fan fill on the MI355X", "",
             "Measured by `tools/bench_mesh_holes.py` (%d training steps, %d rounds, the first untimed; medians of `stats.ms`, min .. max in the JSON beside this file)." % (
                 res["train_steps"], res["rounds"]),
             "`loops` = `DeviceMesh.boundary_loops(edges=True, table=True)`, `fill` = `DeviceMesh.fill_holes()`, `topology` = `DeviceMesh.topology()` on the same mesh,",
             "`reference` = `tests/mesh_holes_reference.expected_fill` on a downloaded copy, once, and whether the device's filled mesh equals it bit for bit.", "",
             "Measured: the wall-clock time of each call as the library reports it (`stats.ms`, allocation and the device-to-host reads of the counts included), the peak",
             "workspace, the loops by size, the census after the fill. Not measured: how a call's time divides between the edge join, the ranking rounds and the emission",
             "(no kernel was timed on its own); the ranking rounds are stated as a count, not as a time. A mesh with 0 boundary edges (the views saw every triangle) measures what",
             "it costs to find that out: the index check, the components, the edge join and one exclusive sum. A mesh that is not closed after the fill holds components that",
             "are not simple loops (random removals that touch in a vertex), which the stage reports and leaves open.", "",
             "| mesh | triangles | boundary edges | loops | loops ms | fill ms | topology ms | reference s | equal bits | peak workspace MB |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        ref = "not run (over the limit)" if r["reference_s"] is None else "%.3f" % r["reference_s"]
        lines.append("| %s | %d | %d | %d | %.3f | %.3f | %.3f | %s | %s | %.1f |" % (r["mesh"], r["n_triangles"], r["loops"]["n_boundary_edges"], r["loops"]["n_loops"], r["loops"]["ms_median"],
                                                                           r["fill"]["ms_median"], r["topology"]["ms_median"], ref, r["equal_bits"], r["fill"]["peak_workspace"] / 1e6))
    names = list(res["results"][0]["loop_sizes"]) if res["results"] else []
    lines += ["", "## Loops", "", "| mesh | simple | irregular vertices | longest | ranking rounds | " + " | ".join("%s edges" % n for n in names) + " |", "|---|---|---|---|---|" + "---|" * len(names)]
    for r in res["results"]:
        s = r["loops"]
        lines.append("| %s | %d | %d | %d | %d | " % (r["mesh"], s["n_simple"], s["n_irregular_vertices"], s["max_loop_edges"], r["ranking_rounds"]) + " | ".join(str(r["loop_sizes"][n]) for n in names) + " |")
    lines += ["", "## Fill", "", "| mesh | filled | not simple | vertices added | triangles added | closed after | oriented after | boundary edges after | Euler before -> after |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        s, a = r["fill"], r["after_fill"]
        lines.append("| %s | %d | %d | %d | %d | %d | %d | %d | %d -> %d |" % (r["mesh"], s["n_filled"], s["n_skipped_not_simple"], s["n_verts_added"], s["n_tris_added"], a["closed"], a["oriented"],
                                                                        a["n_boundary_edges"], r["topology"]["euler"], a["euler"]))
    return "\n".join(lines) + "\n"


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--punch", type=float, default=0.01)
    ap.add_argument("--reference-limit", type=int, default=300000)
    ap.add_argument("--markdown", default=None)
    args = common.parse_args(ap)

    c, scene, train_s = common.train_scene(args)
    views = scene[0]
    results = []
    for r in args.resolution:
        with c.extract_mesh_device(r, colors=True) as m, m.cull_unseen(views, unit="faces") as seen:
            row = dict(mesh="%d^3 extraction, seen faces" % r, resolution=r, punched=0.0, **measure(c, seen, args.rounds, args.reference_limit))
            results.append(row)
            print(json.dumps(row), file=sys.stderr)
            d = seen.download()
            tris = d["indices"].reshape(-1, 3)
            keep = np.random.default_rng(r).random(len(tris)) >= args.punch
            with c.upload_mesh(d["verts"], tris[keep].ravel(), d.get("colors")) as punched:
                row = dict(mesh="%d^3 extraction, seen faces, %g %% of the triangles removed" % (r, 100 * args.punch), resolution=r, punched=args.punch,
                           **measure(c, punched, args.rounds, args.reference_limit))
            results.append(row)
            print(json.dumps(row), file=sys.stderr)

    res = dict(metric="mesh_holes_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, punch=args.punch, results=results)
    common.report(res, args.out)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(res))
    c.close()


if __name__ == "__main__":
    main()
