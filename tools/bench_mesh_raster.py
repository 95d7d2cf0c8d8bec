#!/usr/bin/env python3
"""Cost of rnb_mesh_raster (include/rnb_mesh_raster.h) on one MI355X, and the mesh-versus-model table it exists for.

Trains the config-4 synthetic scene (64 views, 800 x 800) to step 2000 in this process (the scene and protocol of tools/bench_mesh_distance.py). Then at each --resolution
R the mesh is extracted (rnb_extract_mesh) and cleaned (rnb_mesh_clean, largest, outward) once, and simplified (quadric placement) on N^3 cells for every N of --cells.
Every one of these device meshes is rasterised into all the training views at their own size: ms per view (stats.ms, the median of the views after one untimed call, and
min .. max), triangles per second, n_small / n_large, fragments per pixel. Beside it: rnb_render's frame time on the same views (median), and, for the cleaned mesh of each
resolution in --caster, the host BVH caster (hostlib.MeshRayCaster.first_hit, one ray per pixel of view 0: the only thing that answered this question before), its build
and its cast timed apart. The table: mean normal angle and mask IoU against the input maps (api.view_normal_metrics, the definitions of build/render) of the model's
render and of every mesh, over every --metric-stride-th view.

  python tools/bench_mesh_raster.py [--steps 2000] [--resolution 512 1024] [--cells 128 256 512] [--metric-stride 4] [--caster 512 1024] [--out profiles/mesh_raster.json]

Prints one JSON line (and writes it to --out when given). profiles/mesh_raster.md is written by hand from that line, as the other profiles are; the share of each kernel in a
call comes from a run of its own under `rocprofv3 --kernel-trace --stats` (e.g. --steps 300 --resolution 1024 --cells 128 --caster --metric-stride 64).
"""
import json
import os
import sys
import time

import numpy as np

import mesh_bench_common as common


def main():
    ap = common.arg_parser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--cells", type=int, nargs="*", default=[128, 256, 512], help="N of the simplifications")
    ap.add_argument("--metric-stride", type=int, default=4, help="the metrics are taken on every n-th view")
    ap.add_argument("--caster", type=int, nargs="*", default=[512, 1024], help="resolutions whose cleaned mesh also goes through the host BVH caster")
    args = common.parse_args(ap)

    from rnb_neus2_amd import api, _abi, hostlib

    c, (views, normals, albedos), train_s = common.train_scene(args)
    n_pix = args.res * args.res
    img = c.device_malloc(n_pix * _abi.MESH_RASTER_CHANNELS * 4)
    metric_views = list(range(0, len(views), max(args.metric_stride, 1)))

    def metrics(image_of):
        rows = [api.view_normal_metrics(image_of(k), views[k], normals[k]) for k in metric_views]
        return {key: round(float(np.mean([r[key] for r in rows])), 4) for key in ("mean_angle_deg", "median_angle_deg", "mask_iou")}

    def download():
        return c.download(img, n_pix * _abi.MESH_RASTER_CHANNELS, np.float32).reshape(args.res, args.res, _abi.MESH_RASTER_CHANNELS)

    # the model's render: frame time on every view, metrics on the chosen ones
    c.render_into(views[0], img)
    render_ms = [c.render_into(v, img)["ms"] for v in views]

    def render_image(k):
        c.render_into(views[k], img)
        return download()

    model = dict(frame_ms=common.spread(render_ms, untimed=0), **metrics(render_image))
    print(json.dumps(dict(model=model)), file=sys.stderr)

    def raster(m, k):
        return m.rasterize(views[k], out_ptr=img)

    def measure(name, m):
        raster(m, 0)  # untimed
        runs = [raster(m, k) for k in range(len(views))]
        ms = common.spread([r["ms"] for r in runs], untimed=0)
        nt = m.n_triangles

        def image_of(k):
            raster(m, k)
            return download()

        row = dict(mesh=name, n_tris=nt, ms_per_view=ms, mtris_per_s=round(nt / ms["median"] / 1e3, 1), n_small=int(np.median([r["n_small"] for r in runs])),
                   n_large=int(np.median([r["n_large"] for r in runs])), n_offscreen=int(np.median([r["n_offscreen"] for r in runs])),
                   fragments_per_pixel=round(float(np.mean([r["n_fragments"] for r in runs])) / n_pix, 4),
                   fragments_per_covered_pixel=round(float(np.mean([r["n_fragments"] / max(r["n_covered"], 1) for r in runs])), 3),
                   n_back_pixels=int(sum(r["n_back_pixels"] for r in runs)), peak_workspace=runs[-1]["peak_workspace"], **metrics(image_of))
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
            cm = m.clean("largest", "outward")
        with cm:
            block = dict(resolution=r, extract_ms=round(m.stats["ms"], 2), clean_ms=round(cm.stats["ms"], 2), meshes=[measure("%d" % r, cm)])
            if r in args.caster:  # the host caster on the same mesh: one ray per pixel of view 0
                host = cm.download()
                t0 = time.perf_counter()
                caster = hostlib.MeshRayCaster(host["verts"], host["indices"].reshape(-1, 3))
                build_s = time.perf_counter() - t0
                x = np.asarray(views[0]["xform"], np.float64)
                ys, xs = np.meshgrid(np.arange(args.res) + 0.5, np.arange(args.res) + 0.5, indexing="ij")
                fx, fy = views[0]["focal_length"]
                d = np.stack([(xs - 0.5 * args.res) / fx, (ys - 0.5 * args.res) / fy, np.ones_like(xs)], -1).reshape(-1, 3) @ x[:, :3].T
                d = np.ascontiguousarray(d)
                o = np.ascontiguousarray(np.broadcast_to(x[:, 3], d.shape))  # (contiguous before the clock starts: first_hit would copy them otherwise)
                t0 = time.perf_counter()
                t, tri = caster.first_hit(o, d)
                block["host_caster"] = dict(build_ms=round(build_s * 1e3, 1), first_hit_ms=round((time.perf_counter() - t0) * 1e3, 1), n_hit=int((tri >= 0).sum()),
                                            omp_num_threads=os.environ.get("OMP_NUM_THREADS"))  # (None: OpenMP's default, every CPU of the machine)
                print(json.dumps(block["host_caster"]), file=sys.stderr)
                del caster, host
            for n in args.cells:
                with cm.simplify(*c.simplify_grid((0, 0, 0), (1, 1, 1), n)) as sm:
                    block["meshes"].append(measure("%d --simplify %d" % (r, n), sm))
        results.append(block)

    res = dict(metric="mesh_raster_ms_per_view", unit="ms", train_steps=args.steps, train_s=round(train_s, 2), views=len(views), image=args.res, metric_views=len(metric_views),
               model_render=model, results=results)
    common.report(res, args.out)
    c.device_free(img)
    c.close()


if __name__ == "__main__":
    main()
