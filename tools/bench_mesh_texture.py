#!/usr/bin/env python3
"""Cost of rnb_mesh_bake_texture (include/rnb_mesh_texture.h) on one MI355X, against the network evaluation it feeds.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_raster.py). Then at each --resolution R
the mesh is extracted (rnb_extract_mesh) and cleaned (rnb_mesh_clean, largest, outward) once, and simplified (quadric placement) on N^3 cells for every N of --cells.
Every one of these device meshes is baked at every S of --size with the maps of --maps: ms per bake (stats.ms: the median of --repeat calls after one untimed call, and
min .. max), texels per second, the block edge the layout chose. A mesh the texture cannot hold is recorded with the library's message (the smallest size that would).

The yardstick is the network alone over the same point count: Context.forward_infer_staged on network inputs built, as the header builds them, from the first 2^20 owned
texels of the same bake's position map and put into COORDS (every batch evaluates those), in the bake's own batches (2^20 points and a remainder), timed on the host around
the launches and a one-word download that waits for them. `outside_network` = 1 - network_ms / bake_ms: what the two
kernels of the stage, the range check, the clearing of the maps, the UV upload and the allocations cost together.

  python tools/bench_mesh_texture.py [--steps 2000] [--resolution 512 1024] [--cells 128 256] [--size 1024 2048 4096] [--maps albedo] [--repeat 5] [--out profiles/mesh_texture.json]

Prints one JSON line (and writes it to --out when given). profiles/mesh_texture.md is written by hand from that line, as the other profiles are.
"""
import json
import sys
import time

import numpy as np

import mesh_bench_common as common

BATCH = 1 << 20  # the bake's default network batch


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--cells", type=int, nargs="*", default=[128, 256], help="N of the simplifications")
    ap.add_argument("--size", type=int, nargs="*", default=[1024, 2048, 4096], help="texels per side")
    ap.add_argument("--maps", nargs="*", default=["albedo"])
    ap.add_argument("--repeat", type=int, default=5)
    args = common.parse_args(ap)

    from rnb_neus2_amd import api

    c, _, train_s = common.train_scene(args)
    capacity = c.buffer("COORDS", read_only=True)[1] // 28

    def network_ms(n_points, position):
        """n_points through the network alone, in batches of at most min(BATCH, the COORDS buffer), at the texels of `position` (the header's recipe for the network input)."""
        step = min(BATCH, capacity)
        v = position[position[..., 3] == 1][:step, :3]
        v = np.resize(v, (step, 3)) if len(v) < step else v  # (repeated when the mesh owns fewer texels than a batch holds)
        d = v - np.float32(0.5)
        coords = np.zeros((step, 7), np.float32)
        coords[:, 0:3] = np.clip(v, 0.0, 1.0)  # (the scene's box is the unit cube)
        coords[:, 4:7] = (d / np.sqrt((d * d).sum(1, keepdims=True)) + np.float32(1.0)) * np.float32(0.5)
        c.put("COORDS", np.nan_to_num(coords))
        sizes = [step] * (n_points // step) + ([n_points % step] if n_points % step else [])
        times = []
        for _ in range(args.repeat + 1):
            c.get("MLP_OUT", 1)
            t0 = time.perf_counter()
            for n in sizes:
                c.forward_infer_staged(n)
            c.get("MLP_OUT", 1)  # waits for the launches
            times.append((time.perf_counter() - t0) * 1e3)
        return common.spread(times)

    def measure(name, m):
        rows = []
        for size in args.size:
            try:
                lay = api.Context.texture_layout(m.n_triangles, size)
                runs = [m.bake_texture(size, maps=tuple(args.maps)) for _ in range(args.repeat + 1)]
            except api.RnbError as e:
                rows.append(dict(mesh=name, n_tris=m.n_triangles, size=size, skipped=str(e)[-120:]))
                print(json.dumps(rows[-1]), file=sys.stderr)
                continue
            ms = common.spread([r["stats"]["ms"] for r in runs])
            n_texels = runs[-1]["stats"]["n_texels"]
            net = network_ms(n_texels, m.bake_texture(size, maps=("position",))["position"]) if n_texels else None
            rows.append(dict(mesh=name, n_tris=m.n_triangles, size=size, block=lay["block"], n_texels=n_texels, n_batches=runs[-1]["stats"]["n_batches"],
                             fill=round(n_texels / float(size * size), 4), bake_ms=ms, mtexels_per_s=round(n_texels / ms["median"] / 1e3, 1) if n_texels else None,
                             network_ms=net, outside_network=round(1.0 - net["median"] / ms["median"], 4) if net else None, peak_workspace=runs[-1]["stats"]["peak_workspace"]))
            print(json.dumps(rows[-1]), file=sys.stderr)
            del runs
        return rows

    results = []
    for r in args.resolution:
        try:
            m = c.extract_mesh_device(r)
        except Exception as e:  # e.g. no memory on a card that others use
            results.append(dict(resolution=r, skipped=str(e)[:200]))
            continue
        with m:
            cm = m.clean("largest", "outward")
        with cm:
            block = dict(resolution=r, extract_ms=round(m.stats["ms"], 2), clean_ms=round(cm.stats["ms"], 2), bakes=measure("%d" % r, cm))
            for n in args.cells:
                with cm.simplify(*c.simplify_grid((0, 0, 0), (1, 1, 1), n)) as sm:
                    block["bakes"] += measure("%d --simplify %d" % (r, n), sm)
        results.append(block)

    res = dict(metric="mesh_texture_bake_ms", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), views=args.views, image=args.res, maps=list(args.maps), repeat=args.repeat,
               network_batch=min(BATCH, capacity), results=results)
    common.report(res, args.out)
    c.close()


if __name__ == "__main__":
    main()
