#!/usr/bin/env python3
"""Cost of simplifying the extracted mesh on one MI355X: rnb_mesh_simplify (include/rnb_mesh_simplify.h) beside the extraction and the cleaning of the same mesh.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_clean.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh, colours) and cleaned (rnb_mesh_clean, largest, outward) once, and for N = R / 4 and R / 8 the cleaned device mesh goes through
rnb_mesh_simplify on N^3 cells over the unit box: stats.ms over --rounds rounds, the first untimed, median and min .. max, with the triangles in and out, the bytes each
kernel has to move, the peak workspace, and the host's save_obj seconds for the full and for the simplified mesh (once each). A resolution whose extraction fails for
lack of memory is reported as such and skipped.
--kernels-only runs one extraction, one cleaning and one simplification per (R, N) and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`.

  python tools/bench_mesh_simplify.py [--steps 2000] [--resolution 512 1024 2048] [--rounds 5] [--placement quadric] [--out profiles/mesh_simplify.json]

Prints one JSON line (and writes it to --out when given).
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_bytes(nv, nt, n_cells, n_cl, nvo, nto, attrs):
    """Bytes each kernel must read + write (compulsory traffic: every array once; a gather through an index is counted as one pass over the array it gathers from; the
    atomics of the two accumulation kernels as one pass over the 152-byte cluster records)."""
    words = (n_cells + 31) // 32
    return {
        "k_mesh_validate": 12 * nt + 4 * nv,
        "k_sp_cells": 4 * nv + 12 * nv * (1 + attrs) + 4 * nv + 4 * words,
        "k_sp_popc": 8 * words,
        "k_sp_members": 8 * nv + 12 * nv * (1 + attrs) + 8 * words + 4 * n_cl + 80 * n_cl,
        "k_sp_quadric": 12 * nt + 12 * nv + 4 * nv + 72 * n_cl,
        "k_sp_tris<count>": 12 * nt + 4 * nv + 4 * n_cl,
        "k_sp_solve": 164 * n_cl + 12 * nvo * (1 + attrs),
        "k_sp_tris<write>": 12 * nt + 4 * nv + 4 * n_cl + 12 * nto,
        "memsets + k_scan_blocks/k_scan_add (3 scans)": 4 * nv + 4 * words + 156 * n_cl + 2 * 8 * words + 2 * 8 * n_cl + 8 * (nt // 256 + 1),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--res", type=int, default=800, help="image resolution of the training views")
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024, 2048])
    ap.add_argument("--divisors", type=int, nargs="*", default=[4, 8], help="N = resolution / divisor")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--placement", default="quadric", choices=["quadric", "mean"])
    ap.add_argument("--no-obj", action="store_true", help="skip the save_obj timings")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic, _abi, meshproc

    views, normals, albedos = synthetic.make_scene(args.views, args.res)
    c = rnb.Context()
    c.init_params()
    c.set_dataset(views, normals, albedos)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        c.train_step()
    train_s = time.perf_counter() - t0

    def extract(r):
        opt = _abi.MeshOptions()
        c._check(c.f.mesh_default_options(C.byref(opt)))
        opt.res[:] = [r, r, r]
        opt.attributes = _abi.MESH_ATTR_COLORS
        m, st = _abi.Mesh(), _abi.MeshStats()
        c._check(c.f.extract_mesh(c._h, None, C.byref(opt), C.byref(m), C.byref(st)))
        return m, st

    def clean(m):
        out, st = _abi.Mesh(), _abi.MeshCleanStats()
        c._check(c.f.mesh_clean(c._h, None, C.byref(m), C.byref(c._clean_options("largest", "outward")), C.byref(out), None, C.byref(st)))
        return out, st

    def simplify(m, n, keep=False):
        out, st = _abi.Mesh(), _abi.MeshSimplifyStats()
        opt = c._simplify_options(*c.simplify_grid((0, 0, 0), (1, 1, 1), n), args.placement)
        c._check(c.f.mesh_simplify(c._h, None, C.byref(m), C.byref(opt), C.byref(out), C.byref(st)))
        host = c._download_mesh(out) if keep else None
        c.f.mesh_free(c._h, C.byref(out))
        return st.as_dict(), host

    def spread(t):
        t = np.asarray(t[1:] if len(t) > 1 else t)  # the first round is untimed
        return dict(ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3))

    def save_obj_s(host, d, name):
        t = time.perf_counter()
        meshproc.save_obj(os.path.join(d, name), meshproc.Mesh(host["verts"], host["indices"].reshape(-1, 3), host.get("colors")))
        return round(time.perf_counter() - t, 3)

    results = []
    for r in args.resolution:
        try:
            m, est = extract(r)
        except Exception as e:  # e.g. 2048^3 on a card that others use
            results.append(dict(resolution=r, skipped=str(e)[:200]))
            continue
        cm, cst = clean(m)
        c.f.mesh_free(c._h, C.byref(m))
        row = dict(resolution=r, extract_ms=round(est.ms, 2), clean_ms=round(cst.ms, 2), n_tris_extracted=cst.n_tris_in, n_tris_cleaned=cst.n_tris_out, simplify=[])
        with tempfile.TemporaryDirectory() as d:
            if not args.kernels_only and not args.no_obj:
                row["save_obj_full_s"] = save_obj_s(c._download_mesh(cm), d, "full.obj")
            for div in args.divisors:
                n = r // div
                runs = [simplify(cm, n, keep=(k == 0 and not args.kernels_only)) for k in range(1 if args.kernels_only else args.rounds)]
                st = runs[-1][0]
                cell = dict(n=n, **spread([x[0]["ms"] for x in runs]), **{k: v for k, v in st.items() if k != "ms"})
                cell["kernel_bytes"] = kernel_bytes(st["n_verts_in"], st["n_tris_in"], n ** 3, st["n_clusters"], st["n_verts_out"], st["n_tris_out"], 1)
                cell["kernel_bytes_total"] = int(sum(cell["kernel_bytes"].values()))
                if not args.kernels_only and not args.no_obj:
                    cell["save_obj_simplified_s"] = save_obj_s(runs[0][1], d, "small.obj")
                row["simplify"].append(cell)
        c.f.mesh_free(c._h, C.byref(cm))
        results.append(row)
        print(json.dumps(row), file=sys.stderr)

    res = dict(metric="mesh_simplify_ms", unit="ms", placement=args.placement, train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, results=results)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    c.close()


if __name__ == "__main__":
    main()
