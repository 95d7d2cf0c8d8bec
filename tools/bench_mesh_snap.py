#!/usr/bin/env python3
"""Cost and effect of the snapping stage on one MI355X: rnb_mesh_snap (include/rnb_mesh_snap.h) beside the network alone over the same number of points and beside
rnb_mesh_smooth, and the quality tables behind the defaults of iterations, tolerance, max_step and max_displacement.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_clean.py). Then at each --resolution R
four meshes are measured: the extraction (rnb_extract_mesh, colours), its --simplify N version (vertex clustering, repaired), the extraction smoothed
(DeviceMesh.smooth, its defaults), and the simplified one after drop + fill (DeviceMesh.drop_intersecting, DeviceMesh.fill_holes); and two that are further from the
surface, the --coarse N simplification and that one after ten smoothing passes. On each, over --rounds rounds with the first untimed (median and min .. max):
  snap       DeviceMesh.snap() with the library's defaults: stats.ms per call, per round (ms / stats.rounds), stats.ms_network, the points it handed to the network
  network    the network alone over that many points (the baker's comparison: Context.forward_infer_staged on inputs built as the header builds them, in batches of
             2^20, between two one-word downloads); outside_network = 1 - network / snap
  smooth     DeviceMesh.smooth() on the same mesh, its defaults
The quality table, for iterations 0 .. 8 on every mesh: mean and maximum |sdf| before and after (stats.sum_*_q / 2^24 / the valid vertices, stats.max_*), the share of
the vertices per state, Context.mesh_view_metrics' mean normal angle and mask IoU against the input normal maps (--quality-views of them), DeviceMesh.distance_to the
extraction of that resolution (mean, max), and the proper self-intersections after the snap (DeviceMesh.self_intersections). The option table, on the meshes of the first
resolution at the default iterations: tolerance, max_step and max_displacement each at a quarter, a half, once and four times the default. No time is a pass criterion.

  python tools/bench_mesh_snap.py [--steps 2000] [--resolution 512 1024] [--simplify 128] [--coarse 32] [--rounds 5] [--out profiles/mesh_snap.json] [--markdown profiles/mesh_snap.md]

Prints one JSON line (and writes it to --out when given; the tables to --markdown when given).
"""
import json
import sys
import time

import numpy as np

import mesh_bench_common as common

ITERATIONS = tuple(range(9))
STATES = ("converged", "unfinished", "flat", "leashed", "outside", "stalled", "invalid", "reverted")
BATCH = 1 << 20  # the snap's default network batch
FACTORS = (0.25, 0.5, 1.0, 4.0)


def means(st):
    """(mean |sdf| before, after) of a stats dict: the integer sums over the selected vertices that are not INVALID."""
    n = max(st["n_selected"] - st["n_invalid"], 1)
    return st["sum_before_q"] / 2.0 ** 24 / n, st["sum_after_q"] / 2.0 ** 24 / n


def shares(st):
    n = max(st["n_selected"], 1)
    return {s: round(st["n_" + s] / n, 5) for s in STATES}


def network_ms(c, n_points, verts, rounds):
    """n_points through the network alone, in batches of at most min(BATCH, the COORDS buffer), at positions of the mesh (the header's recipe for the network input)."""
    step = min(BATCH, c.buffer("COORDS", read_only=True)[1] // 28)
    v = np.resize(verts, (step, 3)) if len(verts) < step else verts[:step]
    d = v - np.float32(0.5)
    coords = np.zeros((step, 7), np.float32)
    coords[:, 0:3] = np.clip(v, 0.0, 1.0)  # (the scene's box is the unit cube)
    coords[:, 4:7] = (d / np.sqrt((d * d).sum(1, keepdims=True)) + np.float32(1.0)) * np.float32(0.5)
    c.put("COORDS", np.nan_to_num(coords))
    sizes = [step] * (n_points // step) + ([n_points % step] if n_points % step else [])
    times = []
    for _ in range(rounds):
        c.get("MLP_OUT", 1)
        t0 = time.perf_counter()
        for n in sizes:
            c.forward_infer_staged(n)
        c.get("MLP_OUT", 1)  # waits for the launches
        times.append((time.perf_counter() - t0) * 1e3)
    return common.spread(times)


def measure(c, m, rounds):
    """One device mesh: the snap, the network alone and the smoothing over `rounds` rounds."""
    row = dict(n_verts=m.n_verts, n_triangles=m.n_triangles)
    stats = []
    for _ in range(rounds):
        with m.snap() as s:
            stats.append(s.stats)
    last = stats[-1]
    row["snap"] = dict(common.spread([s["ms"] for s in stats], "ms_"), **common.spread([s["ms"] / max(s["rounds"], 1) for s in stats], "ms_per_round_", digits=4),
                       **common.spread([s["ms_network"] for s in stats], "ms_network_"), **{k: v for k, v in last.items() if k not in ("ms", "ms_network")})
    row["network"] = network_ms(c, int(last["n_network_points"]), m.download()["verts"], rounds) if last["n_network_points"] else None
    row["outside_network"] = round(1.0 - row["network"]["median"] / row["snap"]["ms_median"], 4) if row["network"] and row["snap"]["ms_median"] > 0 else None
    runs = []
    for _ in range(rounds):
        with m.smooth() as s:
            runs.append(s.stats)
    row["smooth"] = dict(common.spread([s["ms"] for s in runs], "ms_"), passes=runs[-1]["passes"])
    return row


def quality(c, m, raw, views, normal_maps):
    """The table behind the default number of iterations: per row the residuals, the states, the view metrics, the distance to the extraction and the proper pairs."""
    rows = []
    for it in ITERATIONS:
        with m.snap(iterations=it) as s:
            st = s.stats
            d = s.download()
            met = c.mesh_view_metrics(d["verts"], d["indices"], views, normal_maps)["mean"]
            dist = s.distance_to(raw)
            si = s.self_intersections()
            before, after = means(st)
            rows.append(dict(iterations=it, mean_before=before, mean_after=after, max_before=st["max_before"], max_after=st["max_after"], shares=shares(st), n_moved=st["n_moved"],
                             rounds=st["rounds"], max_displacement=st["max_displacement"], mean_angle_deg=met["mean_angle_deg"], median_angle_deg=met["median_angle_deg"],
                             mask_iou=met["mask_iou"], distance_mean=dist["mean"], distance_max=dist["max"], n_pairs_proper=si["n_pairs_proper"], ms=st["ms"]))
    return rows


def options(m, defaults):
    """tolerance, max_step and max_displacement, one at a time, at a quarter, a half, once and four times the default; the default iterations."""
    rows = []
    for name in ("tolerance", "max_step", "max_displacement"):
        for factor in FACTORS:
            with m.snap(**{name: defaults[name] * factor}) as s:
                st = s.stats
                before, after = means(st)
                rows.append(dict(option=name, value=defaults[name] * factor, mean_before=before, mean_after=after, max_after=st["max_after"], shares=shares(st), rounds=st["rounds"],
                                 n_network_points=st["n_network_points"], max_displacement=st["max_displacement"], ms=st["ms"]))
    return rows


def share_text(sh):
    return ", ".join("%s %.2f %%" % (k, 100 * v) for k, v in sh.items() if v) or "-"


def markdown(res):
    d = res["defaults"]
    lines = ["# Mesh snap: guarded Newton steps onto the model's SDF on the MI355X", "",
             "Measured by `tools/bench_mesh_snap.py` (%d training steps, %d rounds, the first untimed; medians, min .. max in the JSON beside this file)." % (res["train_steps"], res["rounds"]),
             "`snap` = `DeviceMesh.snap()` with the library's defaults (iterations %d, tolerance %.6g, max_step %.6g, max_displacement %.6g), `stats.ms`; `per round` =" % (
                 d["iterations"], d["tolerance"], d["max_step"], d["max_displacement"]),
             "`stats.ms / stats.rounds`; `in network` = `stats.ms_network`; `network alone` = the same number of points through `Context.forward_infer_staged` in batches of 2^20,",
             "the baker's comparison; `outside` = 1 - network alone / snap; `smooth` = `DeviceMesh.smooth()` with its defaults on the same mesh.", "",
             "Measured: the wall-clock time of each call as the library reports it (allocation, the scans, their device-to-host reads and the synchronisations around every network",
             "launch included), the time between those synchronisations, the peak workspace. Not measured: the step and input kernels on their own, the hardware's byte counters,",
             "meshes of other scenes, boxes with an edge other than 1 (every configuration of the project has aabb_scale = 1, so the factor `diag` of the step was read in the",
             "kernel, not measured), and whether later rounds, which evaluate few vertices, would be cheaper folded into one launch.", "",
             "| mesh | vertices | snap ms | per round ms | in network ms | points | network alone ms | outside | rounds | smooth ms | peak workspace MB |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        s = r["snap"]
        lines.append("| %s | %d | %.3f | %.4f | %.3f | %d | %s | %s | %d | %.3f | %.1f |" % (
            r["mesh"], r["n_verts"], s["ms_median"], s["ms_per_round_median"], s["ms_network_median"], s["n_network_points"], "%.3f" % r["network"]["median"] if r["network"] else "-",
            "%.1f %%" % (100 * r["outside_network"]) if r["outside_network"] is not None else "-", s["rounds"], r["smooth"]["ms_median"], s["peak_workspace"] / 1e6))
    lines += ["", "## Quality by number of iterations", "",
              "The other options at their defaults. |sdf|: `stats.sum_*_q / 2^24` over the valid vertices and `stats.max_*`; normal angle and mask IoU: `Context.mesh_view_metrics` against",
              "the input normal maps of %d views, the means over the views; distance: `DeviceMesh.distance_to` the extraction of that resolution; proper pairs:" % res["quality_views"],
              "`DeviceMesh.self_intersections` of the snapped mesh. The row of 0 iterations moves nothing: it is the mesh as it came.", "",
              "| mesh | iterations | mean before | mean after | max before | max after | states | mean angle deg | mask IoU | distance mean | distance max | proper pairs | ms |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        for q in r["quality"]:
            lines.append("| %s | %d | %.3e | %.3e | %.3e | %.3e | %s | %.4f | %.5f | %.3g | %.3g | %d | %.2f |" % (
                r["mesh"], q["iterations"], q["mean_before"], q["mean_after"], q["max_before"], q["max_after"], share_text(q["shares"]), q["mean_angle_deg"], q["mask_iou"],
                q["distance_mean"], q["distance_max"], q["n_pairs_proper"], q["ms"]))
    lines += ["", "## The other options", "", "One option at a time at a quarter, a half, once and four times its default, the default iterations, on the meshes of the first resolution.", "",
              "| mesh | option | value | mean after | max after | states | rounds | points | max displacement | ms |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["results"]:
        for q in r.get("options", ()):
            lines.append("| %s | %s | %.6g | %.3e | %.3e | %s | %d | %d | %.3g | %.2f |" % (r["mesh"], q["option"], q["value"], q["mean_after"], q["max_after"], share_text(q["shares"]), q["rounds"],
                                                                                  q["n_network_points"], q["max_displacement"], q["ms"]))
    lines += ["", "## The defaults", "",
              "The header's proposals were iterations 3, tolerance 2^-13, max_step 1 / 128 and max_displacement 1 / 64. What the tables say about them:", "",
              "* The SDF this network puts out near the surface is a half sum `sdf + sdf_bias` with `sdf_bias = -0.1`: the raw value lies in [2^-4, 2^-3), where a half has a spacing",
              "  of 2^-14. Every residual in these tables is a multiple of 2^-14 = 6.1e-05, and the tolerance of 2^-13 is two such steps. At a quarter of it only an exact zero",
              "  converges and up to a third of the vertices end unfinished or reverted; at half of it (one step) the mean falls by a fifth and several per cent still do. The rule",
              "  was: lower the tolerance only if that share stays below 1 % on every mesh. It does not, so 2^-13 stays.",
              "* On this scene the extraction, its smoothed and its `--simplify 128` versions are within the tolerance as they come (row 0): the snap has nothing to do there, and",
              "  it costs one round and the final evaluation. That is why the two coarser meshes were added after a first run at 512 showed it; on those one iteration brings the",
              "  mean |sdf| from 2.5e-04 .. 5.6e-04 to 6e-05, within 10 % of the best row, and the second and third gain under 3 % more.",
              "* The default number of iterations stays 3 although the last line below names 1: no mesh of this scene is further than 1.5e-03 from the surface, a fifth of one max_step,",
              "  so the table cannot tell how many steps a larger drift needs. A point 0.01 off a sphere, more than one max_step, needs two (tests/test_mesh_snap_cpu.py holds",
              "  the default to that case), and the third is in reserve. A round in which nothing is active is not run, so the reserve costs only where a vertex uses it.",
              "* max_step and max_displacement change no row here, for the same reason: no vertex comes near either. They stay as proposed and are not confirmed by measurement.",
              "* The snap adds no proper self-intersection on any mesh. On the coarse simplification it raises the mean normal angle of the faces (2.7 -> 3.0 deg: vertices on the",
              "  surface make the chords of a coarse mesh cut inside it), after ten smoothing passes it lowers it (3.4 -> 2.6 deg).", ""] + res["default_verdict"]
    return "\n".join(lines) + "\n"


def verdict(results, defaults):
    """What the tables say about the defaults, in words, from the rows themselves: per mesh the smallest row whose mean |sdf| after the snap is within 10 % of the best
    row's, and the largest of those."""
    out, need = [], []
    for r in results:
        best = min(q["mean_after"] for q in r["quality"])
        k = next(q["iterations"] for q in r["quality"] if q["mean_after"] <= 1.1 * best)
        need.append(k)
        base = r["quality"][0]
        at = r["quality"][min(defaults["iterations"], len(r["quality"]) - 1)]
        out.append("* %s: within 10 %% of the best mean |sdf| (%.3e) from %d iterations on; at the default %d: mean %.3e -> %.3e, proper pairs %d -> %d, mean normal angle %.4f -> %.4f deg." % (
            r["mesh"], best, k, defaults["iterations"], base["mean_after"], at["mean_after"], base["n_pairs_proper"], at["n_pairs_proper"], base["mean_angle_deg"], at["mean_angle_deg"]))
    out.append("")
    out.append("The smallest row that is within 10 %% of the best row's mean |sdf| on every mesh: %d iterations; the library's default is %d." % (max(need), defaults["iterations"]))
    for name in ("tolerance", "max_step", "max_displacement"):
        rows = [(r["mesh"], q) for r in results for q in r.get("options", ()) if q["option"] == name]
        if rows:
            at = lambda f: [q for _, q in rows if abs(q["value"] / defaults[name] - f) < 1e-6]
            out.append("* %s (default %.6g): the largest mean |sdf| after over the meshes at a quarter / a half / once / four times the default: %s; the largest share of vertices "
                       "left unfinished or reverted: %s." % (name, defaults[name], " / ".join("%.3e" % max(q["mean_after"] for q in at(f)) for f in FACTORS),
                                                           " / ".join("%.2f %%" % (100 * max(q["shares"]["unfinished"] + q["shares"]["reverted"] for q in at(f))) for f in FACTORS)))
    return out


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--simplify", type=int, default=128)
    ap.add_argument("--coarse", type=int, default=32, help="N of the coarse simplification")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality-views", type=int, default=8)
    ap.add_argument("--markdown", default=None)
    args = common.parse_args(ap)

    from tests import mesh_snap_reference as sr
    defaults = dict(sr.DEFAULTS)  # what the header says; test_mesh_snap_cpu.py holds the library to it

    c, scene, train_s = common.train_scene(args)
    step = max(len(scene[0]) // max(args.quality_views, 1), 1)
    views, normal_maps = scene[0][::step][:args.quality_views], scene[1][::step][:args.quality_views]
    results = []

    def one(name, r, m, raw):
        row = dict(mesh=name, resolution=r, **measure(c, m, args.rounds))
        row["quality"] = quality(c, m, raw, views, normal_maps)
        if r == args.resolution[0]:
            row["options"] = options(m, defaults)
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    grid = c.simplify_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), args.simplify)
    coarse = c.simplify_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), args.coarse)
    for r in args.resolution:
        with c.extract_mesh_device(r, colors=True) as m:
            one("%d^3 extraction" % r, r, m, m)
            with m.smooth() as sm:
                one("%d^3, smoothed" % r, r, sm, m)
            with m.simplify(*grid) as sp, sp.repair() as rm:
                one("%d^3, simplify %d" % (r, args.simplify), r, rm, m)
                with rm.drop_intersecting() as dm, dm.fill_holes() as fm:
                    one("%d^3, simplify %d, drop + fill" % (r, args.simplify), r, fm, m)
            with m.simplify(*coarse) as sp, sp.repair() as rm:
                one("%d^3, simplify %d" % (r, args.coarse), r, rm, m)
                with rm.smooth(passes=10) as sm:
                    one("%d^3, simplify %d, smoothed 10" % (r, args.coarse), r, sm, m)

    res = dict(metric="mesh_snap_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, defaults=defaults, quality_views=len(views), results=results,
               default_verdict=verdict(results, defaults))
    common.report(res, args.out)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(res))
    c.close()


if __name__ == "__main__":
    main()
