#!/usr/bin/env python3
"""Cost of mesh extraction on one MI355X: the dense path (rnb_sdf_lattice + rnb_marching_cubes) against the sparse extractor (include/rnb_mesh.h).

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process and reports how full the trained occupancy bitfield is. Then, interleaved
in the same process (A B C A B C ..., --rounds rounds, the first untimed; medians and the spread max - min reported), it times at each --resolution
  A  rnb_sdf_lattice + rnb_marching_cubes (Context.sdf_lattice + Context.marching_cubes: the mesh is downloaded),
  B  rnb_extract_mesh with cull = NONE,
  C  rnb_extract_mesh with cull = OCCUPANCY,
for every --brick, and B / C alone at the --sparse-only resolutions (where the dense path's 16 bytes per lattice point do not fit or its 2^32 limit applies).

  python tools/bench_mesh.py [--steps 2000] [--resolution 512 1024] [--sparse-only 2048] [--brick 16 32] [--rounds 5] [--out profiles/mesh_sparse.json]

Prints one JSON line (and writes it to --out when given).
"""
import json
import sys
import time

import numpy as np

import mesh_bench_common as common


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--sparse-only", type=int, nargs="*", default=[2048])
    ap.add_argument("--brick", type=int, nargs="*", default=[16, 32])
    ap.add_argument("--rounds", type=int, default=5)
    args = common.parse_args(ap)

    from rnb_neus2_amd import _abi

    c, (views, normals, albedos), train_s = common.train_scene(args)
    bits = c.get("DENSITY_BITFIELD")
    n0 = _abi.GRIDSIZE ** 3 // 8
    fill = float(np.unpackbits(bits[:n0]).mean())  # cascade 0: the only one the unit box consults

    def dense(r):
        t = time.perf_counter()
        ptr = c.sdf_lattice(r)
        verts, idx = c.marching_cubes(ptr, r)
        ms = (time.perf_counter() - t) * 1e3
        c.device_free(ptr)
        return ms, dict(n_verts=len(verts), n_triangles=len(idx) // 3)

    def sparse(r, cull, brick):
        t = time.perf_counter()
        m = c.extract_mesh_device(r, cull=cull, brick=brick)
        ms = (time.perf_counter() - t) * 1e3
        with m:
            info = dict(m.stats, n_verts=m.n_verts, n_triangles=m.n_triangles)
        info.pop("ms")
        return ms, info

    def summary(times, info):
        t = times[1:] if len(times) > 1 else times  # the first round is untimed
        return dict(info, **common.spread(times, "ms_", digits=2), spread_ms=round(max(t) - min(t), 2))

    results = []
    for r, with_dense in [(r, True) for r in args.resolution] + [(r, False) for r in args.sparse_only]:
        legs = ([("dense", lambda r=r: dense(r))] if with_dense else [])
        for b in args.brick:
            legs.append(("none_brick%d" % b, lambda r=r, b=b: sparse(r, "none", b)))
            legs.append(("occupancy_brick%d" % b, lambda r=r, b=b: sparse(r, "occupancy", b)))
        if not with_dense:
            legs = [l for l in legs if l[0].startswith("occupancy")]  # cull = NONE holds 2 bytes for every lattice point: 17 GB at 2048, left out
        times, infos = {k: [] for k, _ in legs}, {}
        for _ in range(args.rounds):
            for k, fn in legs:
                ms, infos[k] = fn()
                times[k].append(ms)
        row = dict(resolution=r)
        for k, _ in legs:
            row[k] = summary(times[k], infos[k])
        results.append(row)
        print(json.dumps(row), file=sys.stderr)

    res = dict(metric="mesh_extraction_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), bitfield_fill_cascade0=round(fill, 4), rounds=args.rounds,
               bricks=args.brick, results=results)
    common.report(res, args.out)
    c.close()


if __name__ == "__main__":
    main()
