#!/usr/bin/env python3
"""Cost of mesh extraction on one MI355X: the dense path (rnb_sdf_lattice + rnb_marching_cubes) against the sparse extractor (include/rnb_mesh.h).

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process and reports how full the trained occupancy bitfield is. Then, interleaved
in the same process (A B C A B C ..., --rounds rounds, the first untimed; medians and the spread max - min reported), it times at each --resolution
  A  rnb_sdf_lattice + rnb_marching_cubes (mesh left on the device, freed),
  B  rnb_extract_mesh with cull = NONE,
  C  rnb_extract_mesh with cull = OCCUPANCY,
for every --brick, and B / C alone at the --sparse-only resolutions (where the dense path's 16 bytes per lattice point do not fit or its 2^32 limit applies).

  python tools/bench_mesh.py [--steps 2000] [--resolution 512 1024] [--sparse-only 2048] [--brick 16 32] [--rounds 5] [--out profiles/mesh_sparse.json]

Prints one JSON line (and writes it to --out when given).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--res", type=int, default=800, help="image resolution of the training views")
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--sparse-only", type=int, nargs="*", default=[2048])
    ap.add_argument("--brick", type=int, nargs="*", default=[16, 32])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic, _abi

    views, normals, albedos = synthetic.make_scene(args.views, args.res)
    c = rnb.Context()
    c.init_params()
    c.set_dataset(views, normals, albedos)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        c.train_step()
    train_s = time.perf_counter() - t0
    bits = c.get("DENSITY_BITFIELD")
    n0 = _abi.GRIDSIZE ** 3 // 8
    fill = float(np.unpackbits(bits[:n0]).mean())  # cascade 0: the only one the unit box consults

    def dense(r):
        t = time.perf_counter()
        ptr = c.sdf_lattice(r)
        pv, pi, nv, ni = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
        res3 = (C.c_uint32 * 3)(r, r, r)
        mn, mx = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
        c._check(c.f.marching_cubes(c._h, None, C.c_void_p(ptr), res3, mn, mx, 0.0, C.byref(pv), C.byref(pi), C.byref(nv), C.byref(ni)))
        ms = (time.perf_counter() - t) * 1e3
        c.device_free(ptr), c.device_free(pv.value), c.device_free(pi.value)
        return ms, dict(n_verts=nv.value, n_triangles=ni.value // 3)

    def sparse(r, cull, brick):
        opt = _abi.MeshOptions()
        c._check(c.f.mesh_default_options(C.byref(opt)))
        opt.res[:] = [r, r, r]
        opt.cull, opt.brick = cull, brick
        m, st = _abi.Mesh(), _abi.MeshStats()
        t = time.perf_counter()
        c._check(c.f.extract_mesh(c._h, None, C.byref(opt), C.byref(m), C.byref(st)))
        ms = (time.perf_counter() - t) * 1e3
        info = dict(st.as_dict(), n_verts=m.n_verts, n_triangles=m.n_indices // 3)
        info.pop("ms")
        c.f.mesh_free(c._h, C.byref(m))
        return ms, info

    def summary(times, info):
        t = np.asarray(times[1:] if len(times) > 1 else times)  # the first round is untimed
        return dict(info, ms_median=round(float(np.median(t)), 2), ms_min=round(float(t.min()), 2), ms_max=round(float(t.max()), 2), spread_ms=round(float(t.max() - t.min()), 2))

    results = []
    for r, with_dense in [(r, True) for r in args.resolution] + [(r, False) for r in args.sparse_only]:
        legs = ([("dense", lambda r=r: dense(r))] if with_dense else [])
        for b in args.brick:
            legs.append(("none_brick%d" % b, lambda r=r, b=b: sparse(r, _abi.MESH_CULL_NONE, b)))
            legs.append(("occupancy_brick%d" % b, lambda r=r, b=b: sparse(r, _abi.MESH_CULL_OCCUPANCY, b)))
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
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    c.close()


if __name__ == "__main__":
    main()
