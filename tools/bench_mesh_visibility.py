#!/usr/bin/env python3
"""Cost of rnb_mesh_visibility (include/rnb_mesh_visibility.h) on one MI355X beside what one had to do before it, and what `build/mesh --keep-seen component` removes.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_raster.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh) and turned outward with every component kept (rnb_mesh_clean all, outward), and simplified (quadric placement) on N^3 cells for
every N of --cells. For every one of these device meshes:
  - DeviceMesh.visibility over all the views in one call, the alpha of the input normal maps as masks: stats.ms of the call and the wall time around it, the records downloaded
    (the median of --rounds calls after one untimed call);
  - the baseline, what answered the question before: one DeviceMesh.rasterize(faces=True) per view into a device image that is not downloaded, the face map downloaded and
    tallied with numpy (bincount of the winners on the mask, per view seen = won >= 1): wall time of the 64 calls and the tally, the same number of rounds;
  - that both give the same n_seen for every triangle;
  - DeviceMesh.cull_unseen(unit="component"): triangles, vertices and components in and out, and the share of the texture atlas that goes with them (the atlas of
    rnb_mesh_bake_texture gives every pair of triangles one block: the share of the triangles is the share of the blocks).

  python tools/bench_mesh_visibility.py [--steps 2000] [--resolution 512 1024] [--cells 128 256] [--rounds 5] [--out profiles/mesh_visibility.json]

Prints one JSON line (and writes it to --out when given). profiles/mesh_visibility.md is written by hand from that line, as the other profiles are.
"""
import json
import sys
import time

import numpy as np

import mesh_bench_common as common


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--cells", type=int, nargs="*", default=[128, 256], help="N of the simplifications")
    ap.add_argument("--rounds", type=int, default=5, help="timed calls of each kind per mesh, after one untimed call")
    args = common.parse_args(ap)

    c, (views, normals, albedos), train_s = common.train_scene(args)
    masks = [np.ascontiguousarray(n[..., 3] > 0) for n in normals]
    n_pix = args.res * args.res
    img = c.device_malloc(n_pix * 9 * 4)

    def device_call(m):
        t0 = time.perf_counter()
        rec, st = m.visibility(views, masks)
        return rec, st, (time.perf_counter() - t0) * 1e3

    def baseline(m):
        """64 rasters, the face maps downloaded, numpy's tally: n_seen per triangle and the milliseconds it took."""
        t0 = time.perf_counter()
        n_seen = np.zeros(m.n_triangles, np.uint32)
        raster_ms = 0.0
        for view, mask in zip(views, masks):
            r = m.rasterize(view, faces=True, out_ptr=img)
            raster_ms += r["ms"]
            f = r["faces"]
            won = np.bincount(f[(f != 0xFFFFFFFF) & mask], minlength=m.n_triangles)  # (the masks have the views' resolution here: the lookup is the identity)
            n_seen += (won >= 1).astype(np.uint32)
        return n_seen, (time.perf_counter() - t0) * 1e3, raster_ms

    def measure(name, m):
        device_call(m), baseline(m)  # untimed
        dev = [device_call(m) for _ in range(args.rounds)]
        base = [baseline(m) for _ in range(args.rounds)]
        rec, st = dev[-1][0], dev[-1][1]
        same = bool(np.array_equal(rec["n_seen"], base[-1][0]))
        call_ms = common.spread([d[1]["ms"] for d in dev], untimed=0)
        wall_ms = common.spread([d[2] for d in dev], untimed=0)
        base_ms = common.spread([b[1] for b in base], untimed=0)
        base_raster_ms = common.spread([b[2] for b in base], untimed=0)
        with m.cull_unseen(views, masks) as kept:
            cs = dict(kept.stats)
        nt = m.n_triangles
        row = dict(mesh=name, n_tris=nt, visibility_call_ms=call_ms, visibility_wall_ms=wall_ms, baseline_wall_ms=base_ms, baseline_raster_ms_sum=base_raster_ms,
                   ratio_baseline_over_device=round(base_ms["median"] / wall_ms["median"], 2), same_n_seen=same, n_faces_seen=st["n_faces_seen"], n_faces_off_mask=st["n_faces_off_mask"],
                   n_small=st["n_small"], n_large=st["n_large"], peak_workspace=st["peak_workspace"],
                   keep_seen_component=dict(n_components=cs["n_components"], n_components_kept=cs["n_components_kept"], n_tris_removed=cs["n_tris_in"] - cs["n_tris_out"],
                                            n_verts_removed=cs["n_verts_in"] - cs["n_verts_out"], atlas_share_removed=round((cs["n_tris_in"] - cs["n_tris_out"]) / max(nt, 1), 6),
                                            select_ms=round(cs["ms"], 3)))
        print(json.dumps(row), file=sys.stderr)
        return row

    results = []
    for r in args.resolution:
        try:
            m = c.extract_mesh_device(r)
        except Exception as e:  # e.g. no memory on a card that others use
            results.append(dict(resolution=r, skipped=str(e)[:200]))
            continue
        with m:
            cm = m.clean("all", "outward")
        with cm:
            block = dict(resolution=r, extract_ms=round(m.stats["ms"], 2), n_components=cm.stats["n_components"], meshes=[measure("%d" % r, cm)])
            for n in args.cells:
                with cm.simplify(*c.simplify_grid((0, 0, 0), (1, 1, 1), n)) as sm:
                    block["meshes"].append(measure("%d --simplify %d" % (r, n), sm))
        results.append(block)

    res = dict(metric="mesh_visibility_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), views=len(views), image=args.res, rounds=args.rounds, results=results)
    common.report(res, args.out)
    c.device_free(img)
    c.close()


if __name__ == "__main__":
    main()
