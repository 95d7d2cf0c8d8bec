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
import json
import os
import sys
import tempfile
import time

import mesh_bench_common as common


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
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024, 2048])
    ap.add_argument("--divisors", type=int, nargs="*", default=[4, 8], help="N = resolution / divisor")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--placement", default="quadric", choices=["quadric", "mean"])
    ap.add_argument("--no-obj", action="store_true", help="skip the save_obj timings")
    ap.add_argument("--kernels-only", action="store_true")
    args = common.parse_args(ap)

    from rnb_neus2_amd import meshproc

    c, (views, normals, albedos), train_s = common.train_scene(args)

    def save_obj_s(host, d, name):
        t = time.perf_counter()
        meshproc.save_obj(os.path.join(d, name), meshproc.Mesh(host["verts"], host["indices"].reshape(-1, 3), host.get("colors")))
        return round(time.perf_counter() - t, 3)

    def simplify(m, n, keep=False):
        with m.simplify(*c.simplify_grid((0, 0, 0), (1, 1, 1), n), placement=args.placement) as out:
            return out.stats, out.download() if keep else None

    results = []
    for r in args.resolution:
        try:
            m = c.extract_mesh_device(r, colors=True)
        except Exception as e:  # e.g. 2048^3 on a card that others use
            results.append(dict(resolution=r, skipped=str(e)[:200]))
            continue
        with m:
            cm = m.clean("largest", "outward")
        with cm, tempfile.TemporaryDirectory() as d:
            cst = cm.stats
            row = dict(resolution=r, extract_ms=round(m.stats["ms"], 2), clean_ms=round(cst["ms"], 2), n_tris_extracted=cst["n_tris_in"], n_tris_cleaned=cst["n_tris_out"], simplify=[])
            if not args.kernels_only and not args.no_obj:
                row["save_obj_full_s"] = save_obj_s(cm.download(), d, "full.obj")
            for div in args.divisors:
                n = r // div
                runs = [simplify(cm, n, keep=(k == 0 and not args.kernels_only)) for k in range(1 if args.kernels_only else args.rounds)]
                st = runs[-1][0]
                cell = dict(n=n, **common.spread([x[0]["ms"] for x in runs], "ms_"), **{k: v for k, v in st.items() if k != "ms"})
                cell["kernel_bytes"] = kernel_bytes(st["n_verts_in"], st["n_tris_in"], n ** 3, st["n_clusters"], st["n_verts_out"], st["n_tris_out"], 1)
                cell["kernel_bytes_total"] = int(sum(cell["kernel_bytes"].values()))
                if not args.kernels_only and not args.no_obj:
                    cell["save_obj_simplified_s"] = save_obj_s(runs[0][1], d, "small.obj")
                row["simplify"].append(cell)
        results.append(row)
        print(json.dumps(row), file=sys.stderr)

    res = dict(metric="mesh_simplify_ms", unit="ms", placement=args.placement, train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, results=results)
    common.report(res, args.out)
    c.close()


if __name__ == "__main__":
    main()
