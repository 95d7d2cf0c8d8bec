#!/usr/bin/env python3
"""Reconstruction pipeline from the command line. The option set is the reference's (run_pipeline.py:27-92), so existing
invocations keep working:

    python run_pipeline.py --input data/scene/ --testbed build/testbed --output out/scene
    python run_pipeline.py --input normals.sfm --testbed build/testbed --albedo-sfm albedos.sfm --mask-sfm masks.sfm --has-albedo
"""
import argparse

import numpy as np

from rnb_neus2_amd.pipeline import run_full_pipeline

SCALING_MODES = ("auto", "pcd", "silhouettes", "silhouettes_v2", "cameras", "none")

# one line per option:  flags | kind | default | what it does        (kind: str / int / float / flag / mode; default "!" = required)
_SPEC = """
--input -i          | str   | !      | where the scene comes from: a folder holding cameras.npz, an .npz, an .sfm or a .json file
--testbed -t        | str   | !      | the training executable (build/testbed)
--output -o         | str   | output | folder that receives the prepared scene, snapshots and meshes
--max-steps         | int   | 10000  | number of training iterations over both stages
--mesh-resolution   | int   | 1024   | lattice size of the final marching-cubes extraction
--scaling-mode      | mode  | auto   | how the scene is brought into the unit sphere
--sphere-scale      | float | 1.0    | radius the normalised scene should fill
--margin-px         | int   | 20     | silhouettes_v2 only: slack around the masks, in pixels
--warmup-ratio      | float | 0.1    | --has-albedo only: share of the iterations spent before the albedos are rescaled
--mask-weight       | float | 1.0    | weight of the silhouette term of the loss
--has-albedo        | flag  |        | train in two phases and rescale the albedo maps in between
--albedo-sfm        | str   |        | SfMData file listing the albedo maps (SfM input)
--mask-sfm          | str   |        | SfMData file listing the masks (SfM input)
--mask-folder       | str   |        | directory of mask images
--supernormal       | flag  |        | SuperNormal variant of the shading loss
--l1                | flag  |        | L1 instead of L2 colour loss
--no-rgbplus        | flag  |        | switch the RGB+ channel off
--n-samples         | int   | 2000   | pixels per view used to estimate the albedo gains
--seed              | int   | 0      | seed of numpy's generator
--device-postprocess | flag |        | clean the final mesh on the GPU (build/mesh --keep largest --orient outward on the stage-2 snapshot) instead of in Python
--mesh-exe          | str   |        | --device-postprocess only: the mesh executable (default: build/mesh beside the testbed)
--simplify          | int   |        | --device-postprocess only: simplify the final mesh on the GPU by vertex clustering on N^3 cells over the scene box (build/mesh --simplify N)
--report-views      | flag  |        | --device-postprocess only: rasterise the final mesh into every input view and write its normal angle and mask IoU per view (build/mesh --report-views)
--texture           | int   |        | --device-postprocess only: bake an albedo texture of S x S texels for the final mesh on the GPU; mesh.mtl and mesh_albedo.png beside mesh.obj (build/mesh --texture S)
--texture-from      | str   |        | --texture only: views = the texture is projected from the input albedo maps through their cameras, the model's albedo where no view reaches (build/mesh --texture-from views)
--keep-seen         | str   |        | --device-postprocess only: drop what no input view sees from the final mesh on the GPU, component (whole connected components) or faces (build/mesh --keep-seen)
--seen-min-views    | int   |        | --keep-seen only: a triangle counts as seen if at least N views see it
--seen-rings        | int   |        | --keep-seen faces only: grow the seen triangles by R rings of neighbours
--seen-masks        | flag  |        | --keep-seen only: the alpha of the input normal maps are the masks
--seen-max-off      | int   |        | --seen-masks only: also drop what lies off the mask in more than N views
--seen-supersample  | int   |        | --keep-seen only: measure at K times the views' resolution
--repair            | flag  |        | --device-postprocess only: repair the final mesh on the GPU after --simplify: degenerate and duplicate triangles go (build/mesh --repair)
--weld              | flag  |        | --repair only: vertices at one position become one vertex first
--duplicates        | str   |        | --repair only: keep, first (build/mesh's default) or cancel
--orient-consistent | flag  |        | --repair only: wind every orientable patch consistently across its shared edges
--report-topology   | flag  |        | --device-postprocess only: print the edge census of the final mesh as one JSON line (build/mesh --report-topology)
--fill-holes        | flag  |        | --device-postprocess only: close the boundary loops of the final mesh on the GPU after --keep-seen and --repair (build/mesh --fill-holes)
--fill-max-edges    | int   |        | --fill-holes only: leave loops of more than N edges open
--fill-skip-largest | flag  |        | --fill-holes only: leave the longest loop of every connected component open
--drop-intersecting | str   |        | --device-postprocess only: remove the self-intersecting triangles of the final mesh on the GPU before --fill-holes, proper or all (build/mesh --drop-intersecting)
--drop-rings        | int   |        | --drop-intersecting only: also remove R rings of triangles around them (0 .. 8)
--report-intersections | flag |      | --device-postprocess only: print the self-intersection census of the final mesh as one JSON line (build/mesh --report-intersections)
--smooth            | int   |        | --device-postprocess only: smooth the final mesh on the GPU by N passes over the one-ring after --fill-holes, Taubin's lambda / mu pairs (build/mesh --smooth N)
--smooth-lambda     | float |        | --smooth only: the factor of the odd passes (0 < L <= 1, build/mesh's default 0.5)
--smooth-mu         | float |        | --smooth only: the factor of the even passes (-1.5 <= M <= 0, build/mesh's default -0.53; 0 = plain Laplacian smoothing)
--smooth-boundary   | str   |        | --smooth only: pin (build/mesh's default), slide or free
--smooth-only-fills | int   |        | --smooth with --fill-holes only: move only the vertices --fill-holes appended and R rings around them
--smooth-normals    | str   |        | --smooth only: keep or recompute
--snap              | int   |        | --device-postprocess only: move the vertices of the final mesh back onto the model's surface on the GPU by up to N guarded Newton steps after --smooth (build/mesh --snap N)
--snap-tolerance    | float |        | --snap only: a vertex is done where the SDF's magnitude is at most T (build/mesh's default 2^-13)
--snap-max-step     | float |        | --snap only: the longest single step in world units (build/mesh's default: the box edge / 128)
--snap-max-displacement | float |    | --snap only: no vertex ends further than D from where it was (build/mesh's default: the box edge / 64)
--snap-only-fills   | flag  |        | --snap with --fill-holes only: snap only the vertices --fill-holes appended and those --smooth moved
--snap-attributes   | str   |        | --snap only: keep or resample (build/mesh's default)
--report-residual   | flag  |        | --device-postprocess only: print mean and maximum SDF magnitude of the final mesh's vertices as one JSON line (build/mesh --report-residual)
"""


def build_parser():
    parser = argparse.ArgumentParser(description="RNb-NeuS2 pipeline on the MI355X training path")
    casts = {"int": int, "float": float}
    for line in _SPEC.strip().splitlines():
        flags, kind, default, text = (field.strip() for field in line.split("|"))
        kw = {"help": text}
        if kind == "flag":
            kw["action"] = "store_true"
        else:
            if kind in casts:
                kw["type"] = casts[kind]
            if kind == "mode":
                kw["choices"] = list(SCALING_MODES)
            if default == "!":
                kw["required"] = True
            else:
                kw["default"] = casts.get(kind, str)(default) if default else (None if kind in casts else "")  # (a number without a default: absent = None)
        parser.add_argument(*flags.split(), **kw)
    return parser


def pipeline_kwargs(ns):
    """argparse namespace -> keywords of rnb_neus2_amd.pipeline.run_full_pipeline."""
    renamed = {"input": "input_path", "testbed": "testbed_path", "output": "output_dir", "supernormal": "super_normal", "l1": "use_l1",
               "albedo_sfm": "albedo_sfm_path", "mask_sfm": "mask_sfm_path", "mask_folder": "mask_folder_path"}
    kw = {renamed.get(k, k): v for k, v in vars(ns).items() if k not in ("seed", "no_rgbplus", "device_postprocess", "mesh_exe", "simplify", "report_views", "texture", "texture_from", "keep_seen", "seen_min_views",
                                                                                "seen_rings", "seen_masks", "seen_max_off", "seen_supersample", "repair", "weld", "duplicates", "orient_consistent",
                                                                                "report_topology", "fill_holes", "fill_max_edges", "fill_skip_largest", "drop_intersecting", "drop_rings",
                                                                                "report_intersections", "smooth", "smooth_lambda", "smooth_mu", "smooth_boundary", "smooth_only_fills", "smooth_normals", "snap", "snap_tolerance",
                                                                                "snap_max_step", "snap_max_displacement", "snap_only_fills", "snap_attributes", "report_residual")}
    kw["use_rgb_plus"] = not ns.no_rgbplus
    if ns.device_postprocess:  # (absent otherwise: the default call is the reference's)
        kw["device_postprocess"] = True
        kw["mesh_exe"] = ns.mesh_exe or None
        if ns.simplify is not None:
            kw["simplify"] = ns.simplify
        if ns.report_views:
            kw["report_views"] = True
        if ns.texture is not None:
            kw["texture"] = ns.texture
        if ns.texture_from:
            kw["texture_from"] = ns.texture_from
        if ns.keep_seen:
            ks = dict(unit=ns.keep_seen, min_views=ns.seen_min_views, rings=ns.seen_rings, masks=ns.seen_masks or None, max_off=ns.seen_max_off, supersample=ns.seen_supersample)
            kw["keep_seen"] = {k: v for k, v in ks.items() if v is not None}
        if ns.repair:
            kw["repair"] = dict(weld=ns.weld, orient_consistent=ns.orient_consistent, **({"duplicates": ns.duplicates} if ns.duplicates else {}))
        if ns.report_topology:
            kw["report_topology"] = True
        if ns.fill_holes:
            kw["fill_holes"] = dict(skip_largest=ns.fill_skip_largest, **({"max_edges": ns.fill_max_edges} if ns.fill_max_edges is not None else {}))
        if ns.drop_intersecting:
            kw["drop_intersecting"] = dict(classes=ns.drop_intersecting, **({"rings": ns.drop_rings} if ns.drop_rings is not None else {}))
        if ns.report_intersections:
            kw["report_intersections"] = True
        if ns.smooth is not None:
            sm = dict(passes=ns.smooth, lam=ns.smooth_lambda, mu=ns.smooth_mu, boundary=ns.smooth_boundary or None, only_fills=ns.smooth_only_fills, normals=ns.smooth_normals or None)
            kw["smooth"] = {k: v for k, v in sm.items() if v is not None}
        if ns.snap is not None:
            sn = dict(iterations=ns.snap, tolerance=ns.snap_tolerance, max_step=ns.snap_max_step, max_displacement=ns.snap_max_displacement, only_fills=ns.snap_only_fills or None,
                      attributes=ns.snap_attributes or None)
            kw["snap"] = {k: v for k, v in sn.items() if v is not None}
        if ns.report_residual:
            kw["report_residual"] = True
    return kw


def main(argv=None):
    parser = build_parser()
    ns = parser.parse_args(argv)
    if ns.mesh_exe and not ns.device_postprocess:
        parser.error("--mesh-exe is only used with --device-postprocess")
    if ns.simplify is not None and not ns.device_postprocess:
        parser.error("--simplify is only used with --device-postprocess")
    if ns.report_views and not ns.device_postprocess:
        parser.error("--report-views is only used with --device-postprocess")
    if ns.texture is not None and not ns.device_postprocess:
        parser.error("--texture is only used with --device-postprocess")
    if ns.texture is not None and not 4 <= ns.texture <= 8192:
        parser.error("--texture must be 4 .. 8192")
    if ns.texture_from and ns.texture is None:
        parser.error("--texture-from is only used with --texture")
    if ns.texture_from and ns.texture_from != "views":
        parser.error("--texture-from must be views")
    if ns.keep_seen and not ns.device_postprocess:
        parser.error("--keep-seen is only used with --device-postprocess")
    if ns.keep_seen and ns.keep_seen not in ("component", "faces"):
        parser.error("--keep-seen must be component or faces")
    for name in ("seen_min_views", "seen_rings", "seen_masks", "seen_max_off", "seen_supersample"):
        if getattr(ns, name) not in (None, False) and not ns.keep_seen:
            parser.error("--%s is only used with --keep-seen" % name.replace("_", "-"))
    if ns.seen_rings is not None and ns.keep_seen != "faces":
        parser.error("--seen-rings is only used with --keep-seen faces")
    if ns.seen_max_off is not None and not ns.seen_masks:
        parser.error("--seen-max-off is only used with --seen-masks")
    if ns.repair and not ns.device_postprocess:
        parser.error("--repair is only used with --device-postprocess")
    if ns.report_topology and not ns.device_postprocess:
        parser.error("--report-topology is only used with --device-postprocess")
    for name in ("weld", "duplicates", "orient_consistent"):
        if getattr(ns, name) and not ns.repair:
            parser.error("--%s is only used with --repair" % name.replace("_", "-"))
    if ns.fill_holes and not ns.device_postprocess:
        parser.error("--fill-holes is only used with --device-postprocess")
    for name in ("fill_max_edges", "fill_skip_largest"):
        if getattr(ns, name) not in (None, False) and not ns.fill_holes:
            parser.error("--%s is only used with --fill-holes" % name.replace("_", "-"))
    if ns.fill_max_edges is not None and ns.fill_max_edges < 3:
        parser.error("--fill-max-edges must be at least 3")
    if (ns.drop_intersecting or ns.report_intersections) and not ns.device_postprocess:
        parser.error("--drop-intersecting and --report-intersections are only used with --device-postprocess")
    if ns.drop_intersecting and ns.drop_intersecting not in ("proper", "all"):
        parser.error("--drop-intersecting must be proper or all")
    if ns.drop_rings is not None and not ns.drop_intersecting:
        parser.error("--drop-rings is only used with --drop-intersecting")
    if ns.drop_rings is not None and not 0 <= ns.drop_rings <= 8:
        parser.error("--drop-rings must be 0 .. 8")
    if ns.smooth is not None and not ns.device_postprocess:
        parser.error("--smooth is only used with --device-postprocess")
    for name in ("smooth_lambda", "smooth_mu", "smooth_boundary", "smooth_only_fills", "smooth_normals"):
        if getattr(ns, name) not in (None, "") and ns.smooth is None:
            parser.error("--%s is only used with --smooth" % name.replace("_", "-"))
    if ns.smooth is not None and not 0 <= ns.smooth <= 10000:
        parser.error("--smooth must be 0 .. 10000")
    if ns.smooth_lambda is not None and not 0.0 < ns.smooth_lambda <= 1.0:
        parser.error("--smooth-lambda must be above 0 and at most 1")
    if ns.smooth_mu is not None and not -1.5 <= ns.smooth_mu <= 0.0:
        parser.error("--smooth-mu must be at least -1.5 and at most 0")
    if ns.smooth_boundary and ns.smooth_boundary not in ("pin", "slide", "free"):
        parser.error("--smooth-boundary must be pin, slide or free")
    if ns.smooth_normals and ns.smooth_normals not in ("keep", "recompute"):
        parser.error("--smooth-normals must be keep or recompute")
    if ns.smooth_only_fills is not None and (not ns.fill_holes or not 0 <= ns.smooth_only_fills <= 1024):
        parser.error("--smooth-only-fills (0 .. 1024) is only used with --fill-holes")
    if (ns.snap is not None or ns.report_residual) and not ns.device_postprocess:
        parser.error("--snap and --report-residual are only used with --device-postprocess")
    for name in ("snap_tolerance", "snap_max_step", "snap_max_displacement", "snap_only_fills", "snap_attributes"):
        if getattr(ns, name) not in (None, "", False) and ns.snap is None:
            parser.error("--%s is only used with --snap" % name.replace("_", "-"))
    if ns.snap is not None and not 0 <= ns.snap <= 64:
        parser.error("--snap must be 0 .. 64")
    if ns.snap_tolerance is not None and not 0.0 <= ns.snap_tolerance < float("inf"):
        parser.error("--snap-tolerance must be finite and at least 0")
    if ns.snap_max_step is not None and not 0.0 < ns.snap_max_step < float("inf"):
        parser.error("--snap-max-step must be finite and above 0")
    if ns.snap_max_displacement is not None and not 0.0 <= ns.snap_max_displacement < float("inf"):
        parser.error("--snap-max-displacement must be finite and at least 0")
    if ns.snap_only_fills and not ns.fill_holes:
        parser.error("--snap-only-fills is only used with --fill-holes")
    if ns.snap_attributes and ns.snap_attributes not in ("keep", "resample"):
        parser.error("--snap-attributes must be keep or resample")
    if ns.duplicates and ns.duplicates not in ("keep", "first", "cancel"):
        parser.error("--duplicates must be keep, first or cancel")
    if ns.simplify is not None and not 1 <= ns.simplify <= 1024:
        parser.error("--simplify must be 1 .. 1024")
    np.random.seed(ns.seed)
    return run_full_pipeline(**pipeline_kwargs(ns))


if __name__ == "__main__":
    main()
