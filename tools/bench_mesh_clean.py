#!/usr/bin/env python3
"""Cost of cleaning the extracted mesh on one MI355X: rnb_mesh_clean (include/rnb_mesh_clean.h) against the Python stage it replaces.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process. Then at each --resolution
  (a) rnb_mesh_clean alone on the device mesh rnb_extract_mesh returned: stats.ms, --rounds rounds, the first untimed, median and spread, beside rnb_mesh_stats.ms of the
      extraction of that mesh (same run) and the bytes each kernel has to move for it;
  (b) Context.extract_mesh(keep="largest") against Context.extract_mesh(), wall clock, interleaved, downloads included;
  (c) the Python stage on the same mesh written as an OBJ: meshproc.load_obj + split + max(area) + fix_normals + save_obj, run ONCE, timed per part
      (--no-python skips it; at 1024 it takes minutes).
--kernels-only runs one extraction and one rnb_mesh_clean per resolution and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`.

  python tools/bench_mesh_clean.py [--steps 2000] [--resolution 512 1024] [--rounds 5] [--no-python] [--out profiles/mesh_clean.json]

Prints one JSON line (and writes it to --out when given).
"""
import json
import os
import sys
import tempfile
import time

import mesh_bench_common as common


def kernel_bytes(nv, nt, nvo, nto, n_comp, attrs):
    """Bytes each kernel must read + write for a mesh of nv vertices and nt triangles (compulsory traffic: every array once; the gathers through an index are counted
    as one pass over the array they gather from)."""
    return {
        "k_cl_init": 4 * nv,
        "k_mesh_validate": 12 * nt + 4 * nv,
        "k_cl_hook": 12 * nt + 4 * nv,
        "k_cl_flatten": 8 * nv,
        "k_cl_roots": 12 * nv,
        "k_cl_relabel": 16 * nv + 4 * n_comp,
        "k_cl_sums<tri>": 12 * nt + 12 * nv + 4 * nv,
        "k_cl_sums<vert>": 4 * nv,
        "k_cl_select": 2 * 32 * n_comp + 4 * n_comp,
        "k_cl_vflag": 8 * nv,
        "k_compact_verts<ClKeep>": 8 * nv + (12 * nv + 12 * nvo) * (1 + attrs),
        "k_compact_tris<count, ClKeep>": 12 * nt + 4 * nv,
        "k_compact_tris<write, ClKeep>": 12 * nt + 8 * nv + 12 * nto,
        "k_scan_blocks/k_scan_add (3 scans)": 2 * (2 * 8 * nv) + 8 * (nt // 256 + 1),
    }


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-python", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    args = common.parse_args(ap)

    from rnb_neus2_amd import meshproc

    c, (views, normals, albedos), train_s = common.train_scene(args)

    results = []
    for r in args.resolution:
        with c.extract_mesh_device(r, colors=True) as m:
            row = dict(resolution=r, extract_ms=round(m.stats["ms"], 2))
            clean = lambda: m.clean("largest", "outward")
            if args.kernels_only:
                with clean() as cm:
                    row["clean"] = cm.stats
                results.append(row)
                continue
            # (a) the device call alone
            runs = []
            for _ in range(args.rounds):
                with clean() as cm:
                    runs.append(cm.stats)
            st = runs[-1]
            row["clean"] = dict(common.spread([x["ms"] for x in runs], "ms_"), **{k: v for k, v in st.items() if k != "ms"})
            row["kernel_bytes"] = kernel_bytes(st["n_verts_in"], st["n_tris_in"], st["n_verts_out"], st["n_tris_out"], st["n_components"], 1)
            row["kernel_bytes_total"] = int(sum(row["kernel_bytes"].values()))
            host = m.download()
        # (b) through the Python interface, downloads included
        plain, kept = [], []
        for _ in range(args.rounds):
            t = time.perf_counter()
            c.extract_mesh(r, colors=True)
            plain.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            c.extract_mesh(r, colors=True, keep="largest")
            kept.append((time.perf_counter() - t) * 1e3)
        row["extract_mesh"] = common.spread(plain, "ms_")
        row["extract_mesh_keep_largest"] = common.spread(kept, "ms_")
        # (c) the Python stage on the same mesh, once
        if not args.no_python:
            with tempfile.TemporaryDirectory() as d:
                src, dst = os.path.join(d, "in.obj"), os.path.join(d, "out.obj")
                meshproc.save_obj(src, meshproc.Mesh(host["verts"], host["indices"].reshape(-1, 3), host["colors"]))
                parts = {}
                t = time.perf_counter()
                mesh = meshproc.load_obj(src)
                parts["load_obj_s"] = time.perf_counter() - t
                t = time.perf_counter()
                comps = mesh.split()
                best = max(comps, key=lambda x: x.area) if len(comps) > 1 else mesh
                parts["split_s"] = time.perf_counter() - t
                t = time.perf_counter()
                best.fix_normals()
                parts["fix_normals_s"] = time.perf_counter() - t
                t = time.perf_counter()
                meshproc.save_obj(dst, best)
                parts["save_obj_s"] = time.perf_counter() - t
                parts["total_s"] = sum(parts.values())
                row["python_stage"] = dict({k: round(v, 3) for k, v in parts.items()}, n_components=len(comps), n_triangles_kept=len(best.faces))
        results.append(row)
        print(json.dumps(row), file=sys.stderr)

    res = dict(metric="mesh_clean_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), rounds=args.rounds, results=results)
    common.report(res, args.out)
    c.close()


if __name__ == "__main__":
    main()
