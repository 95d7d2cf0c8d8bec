#!/usr/bin/env python3
"""Evaluate a reconstructed mesh against a reference mesh on the device: Chamfer distance, Hausdorff distance, precision, recall and F-score (rnb_mesh_distance,
include/rnb_mesh_distance.h, once per direction).

  python tools/mesh_eval.py --mesh A.obj --reference B.obj [--tau T ...] [--max-distance D] [--level L] [--weld]

Both files are read by meshproc.load_obj. Conventions (those of Context.mesh_distance): each surface is sampled at the centroids of the 4^L congruent sub-triangles of
every triangle, weighted with their areas; accuracy = the mean distance mesh -> reference, completeness = reference -> mesh, chamfer = their sum (unsquared distances, not
halved), hausdorff = the larger of the two maxima; per threshold tau, precision = the area fraction of the mesh within tau of the reference, recall = the area fraction of
the reference within tau of the mesh, fscore = 2 P R / (P + R). Without --tau the thresholds are 0.5 % and 1 % of the diagonal of the reference's bounding box. The sums
are kept in units of 2^k, the power of two next below the diagonal / 1024 (the `unit` of the call: it scales the fixed-point sums and changes no distance).
--max-distance caps every distance (outliers then count as D). --weld: both meshes first go through rnb_mesh_repair (include/rnb_mesh_topology.h) with weld alone --
vertices at one position become one, no triangle is removed -- so that an OBJ that splits its vertices per corner is measured as the surface it draws, not as triangle
soup; the distances do not change by it, `welded` reports the vertices merged per mesh.

Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def choose_unit(diagonal):
    """The power of two next below diagonal / 1024."""
    if not (diagonal > 0 and math.isfinite(diagonal)):
        raise ValueError("the reference has no extent")
    return 2.0 ** math.floor(math.log2(diagonal / 1024.0))


def evaluate(ctx, mesh, reference, taus=(), max_distance=0.0, level=1, weld=False):
    """mesh, reference: (verts float[n,3], faces int[m,3]). The dict this program prints."""
    welded = None
    if weld:
        fixed = [ctx.repair_mesh(m[0], m[1], weld=True, duplicates="keep", drop_degenerate=False) for m in (mesh, reference)]
        mesh, reference = [(m["verts"], m["indices"].reshape(-1, 3)) for m in fixed]
        welded = [m["stats"]["n_welded"] for m in fixed]
    rv = np.asarray(reference[0], np.float32).reshape(-1, 3)
    used = np.unique(np.asarray(reference[1]).ravel())
    diagonal = float(np.linalg.norm(rv[used].max(0).astype(np.float64) - rv[used].min(0).astype(np.float64))) if len(used) else 0.0
    unit = choose_unit(diagonal)
    taus = [float(t) for t in taus] or [0.005 * diagonal, 0.01 * diagonal]
    r = ctx.mesh_distance(mesh[0], mesh[1], reference[0], reference[1], level=level, max_distance=max_distance, unit=unit, thresholds=taus, symmetric=True)
    back = r["reverse"]
    return dict(chamfer=r["chamfer"], hausdorff=r["hausdorff"], accuracy=r["mean"], completeness=back["mean"], accuracy_rms=r["rms"], completeness_rms=back["rms"],
                tau=taus, precision=r["within"], recall=back["within"], fscore=r["fscore"], unit=unit, diagonal=diagonal, level=level, max_distance=max_distance,
                n_samples=[r["n_samples"], back["n_samples"]], n_beyond=[r["n_beyond"], back["n_beyond"]], quantisation=[r["quantisation"], back["quantisation"]],
                ms=[r["ms"], back["ms"]], **({} if welded is None else dict(welded=welded)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True, help="the reconstruction (.obj)")
    ap.add_argument("--reference", required=True, help="the ground truth (.obj)")
    ap.add_argument("--tau", type=float, nargs="*", default=[], help="up to four thresholds, in the units of the files")
    ap.add_argument("--max-distance", type=float, default=0.0)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--weld", action="store_true", help="weld vertices at one position in both meshes first")
    args = ap.parse_args(argv)
    if len(args.tau) > 4 or any(not t > 0 for t in args.tau):
        ap.error("--tau takes up to four positive thresholds")

    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import meshproc
    a, b = meshproc.load_obj(args.mesh), meshproc.load_obj(args.reference)
    with rnb.Context() as c:
        out = evaluate(c, (a.vertices, a.faces), (b.vertices, b.faces), args.tau, args.max_distance, args.level, args.weld)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
