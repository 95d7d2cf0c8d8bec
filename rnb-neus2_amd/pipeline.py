"""Pipeline orchestration around the `testbed` executable (mirror of rnb_neus2/pipeline.py: same entry points, same
arguments, same testbed command lines — pinned against the reference's own by tests/golden/pipeline_argv.json).

Structure: every workflow is first *planned* as a list of `Stage`s (argv + what it must leave behind), then executed.
The plan functions are pure, which is what the tests compare with the recorded reference behaviour."""
import os
import shutil
import subprocess
from dataclasses import dataclass, field
from pathlib import Path
from typing import List


class SimpleLogger:
    def info(self, msg):
        print("[INFO] {}".format(msg))

    def warning(self, msg):
        print("[WARN] {}".format(msg))

    def error(self, msg):
        print("[ERROR] {}".format(msg))


@dataclass
class Stage:
    name: str
    max_iter: int
    flags: List[str] = field(default_factory=list)

    def argv(self, testbed_path, scene_path):
        return [testbed_path, "--scene", str(scene_path) + "/", "--maxiter", str(self.max_iter), "--no-gui"] + list(self.flags)


def stage1_iterations(max_steps):
    return int(max_steps * 2 / 3)  # pipeline.py:63


def warmup_iterations(max_steps, warmup_ratio):
    return max(int(max_steps * warmup_ratio), 1000)  # pipeline.py:116


def snapshot_candidates(data_dir, iters):
    """Where a stage's snapshot is looked for, in order. (pipeline.py:77-85)"""
    name = "snapshot_{}.msgpack".format(iters)
    return [os.path.join(data_dir, "output", name), os.path.join(data_dir, name)]


def common_flags(mask_weight=1.0, super_normal=False, use_l1=False, use_rgb_plus=True):
    """run_full_pipeline's keyword -> flag mapping. (pipeline.py:281-288)"""
    flags = ["--mask-weight", str(mask_weight)]
    if super_normal:
        flags.append("--supernormal")
    if use_l1:
        flags.append("--lone")
    if not use_rgb_plus:
        flags.append("--no-rgbplus")
    return flags


def plan_two_stage(data_dir, max_steps, flags, resolution=1024, no_albedo=False, extra_flags=None):
    """Stage 1 trains 2/3 of the budget and saves a snapshot; stage 2 resumes from it with optimal lights up to
    `max_steps`, then meshes. (pipeline.py:56-103)"""
    tail = (["--no-albedo"] if no_albedo else []) + list(extra_flags or [])
    it1 = stage1_iterations(max_steps)
    snapshot = snapshot_candidates(data_dir, it1)[0]
    return [Stage("Stage 1", it1, list(flags) + ["--save-snapshot"] + tail),
            Stage("Stage 2", max_steps, list(flags) + ["--opti-lights", "--snapshot", snapshot, "--resolution", str(resolution), "--save-mesh", "--save-snapshot", "--free-memory"] + tail)]


def plan_warmup(max_steps, flags, warmup_ratio=0.1):
    """Geometry-only phase before albedo scaling: normals only, 512^3 mesh. (pipeline.py:116-128)"""
    return Stage("Phase 1 (warmup)", warmup_iterations(max_steps, warmup_ratio), list(flags) + ["--no-albedo", "--save-mesh", "--resolution", "512", "--free-memory"])


def run_testbed(testbed_path, scene_path, max_iter, flags, stage_name, logger=None):
    """One testbed process; stdout is relayed line by line, a non-zero exit raises. (pipeline.py:27-53)"""
    logger = logger or SimpleLogger()
    cmd = Stage(stage_name, max_iter, list(flags)).argv(testbed_path, scene_path)
    logger.info("{} command: {}".format(stage_name, " ".join(cmd)))
    result = subprocess.run(cmd, capture_output=True, text=True)
    if result.stdout:
        for line in result.stdout.strip().split("\n"):
            logger.info(line)
    if result.returncode != 0:
        if result.stderr:
            logger.error(result.stderr)
        raise RuntimeError("{} failed with code {}".format(stage_name, result.returncode))
    logger.info("{} completed".format(stage_name))


def run_two_stage(testbed_path, data_dir, max_steps, common_flags, resolution=1024, no_albedo=False, extra_flags=None, logger=None):
    logger = logger or SimpleLogger()
    first, second = plan_two_stage(data_dir, max_steps, common_flags, resolution, no_albedo, extra_flags)
    logger.info("Stage 1: {} iterations".format(first.max_iter))
    run_testbed(testbed_path, data_dir, first.max_iter, first.flags, first.name, logger)
    found = [p for p in snapshot_candidates(data_dir, first.max_iter) if os.path.exists(p)]
    if not found:
        raise RuntimeError("Snapshot not found after {} iterations".format(first.max_iter))
    second.flags[second.flags.index("--snapshot") + 1] = found[0]
    logger.info("Stage 2: {} iterations (opti-lights)".format(max_steps))
    run_testbed(testbed_path, data_dir, second.max_iter, second.flags, second.name, logger)


def find_phase1_mesh(data_dir, warmup_steps):
    """mesh_<steps>.obj in <data_dir>/output, else the newest mesh_*.obj there. (pipeline.py:131-141)"""
    out = os.path.join(data_dir, "output")
    path = os.path.join(out, "mesh_{}.obj".format(warmup_steps))
    if os.path.exists(path):
        return path
    candidates = list(Path(out).glob("mesh_*.obj"))
    if not candidates:
        raise RuntimeError("Phase 1 mesh not found in {}".format(out))
    return str(max(candidates, key=lambda p: p.stat().st_mtime))


def run_with_albedo_scaling(testbed_path, data_dir, max_steps, common_flags, resolution=1024, warmup_ratio=0.1, n_samples=2000, logger=None):
    """Warm-up (geometry) -> per-view albedo gains from the warm-up mesh -> albedos/ replaced by the scaled set and the
    warm-up output removed -> the two-stage run with albedo. (pipeline.py:106-175)"""
    logger = logger or SimpleLogger()
    from .albedo_scaling import compute_albedo_scale_ratios, scale_and_save_albedos

    warm = plan_warmup(max_steps, common_flags, warmup_ratio)
    logger.info("=== Phase 1: Geometry only ({} steps) ===".format(warm.max_iter))
    run_testbed(testbed_path, data_dir, warm.max_iter, warm.flags, warm.name, logger)
    mesh_path = find_phase1_mesh(data_dir, warm.max_iter)
    logger.info("=== Albedo scaling ===")
    albedo_dir, scaled_dir = os.path.join(data_dir, "albedos"), os.path.join(data_dir, "albedos_scaled")
    ratios = compute_albedo_scale_ratios(albedo_path=albedo_dir, camera_source=os.path.join(data_dir, "transform.json"), mesh_path=mesh_path, n_samples=n_samples, logger=logger)
    scale_and_save_albedos(albedo_path=albedo_dir, output_albedo_path=scaled_dir, scale_ratios=ratios, logger=logger)
    shutil.rmtree(albedo_dir)
    os.rename(scaled_dir, albedo_dir)
    logger.info("Albedos scaled and replaced")
    shutil.rmtree(os.path.join(data_dir, "output"), ignore_errors=True)
    logger.info("=== Phase 3: Full training with scaled albedos ===")
    run_two_stage(testbed_path, data_dir, max_steps, common_flags, resolution=resolution, logger=logger)


def find_output_mesh(data_dir):
    """Newest mesh_*.o* in <data_dir>/output, else in <data_dir> (json/txt/msgpack excluded). (pipeline.py:185-198)"""
    out = os.path.join(data_dir, "output")
    files = list(Path(out).glob("mesh_*.o*")) if os.path.isdir(out) else []
    if not files:
        files = list(Path(data_dir).glob("mesh_*.o*"))
    files = [f for f in files if f.suffix not in (".json", ".txt", ".msgpack")]
    if not files:
        raise RuntimeError("No mesh files in {} or {}".format(out, data_dir))
    return max(files, key=lambda p: p.stat().st_mtime)


def postprocess_mesh(data_dir, output_mesh_path, logger=None):
    """Keep the largest connected component (by area), orient normals outward, export OBJ, drop the training output
    directory. (pipeline.py:178-219)"""
    logger = logger or SimpleLogger()
    from .meshproc import load_obj, save_obj

    mesh_file = find_output_mesh(data_dir)
    logger.info("Post-processing: {}".format(mesh_file.name))
    mesh = load_obj(str(mesh_file))
    parts = mesh.split()
    if len(parts) > 1:
        mesh = max(parts, key=lambda m: m.area)
        logger.info("Kept largest component ({} vertices)".format(len(mesh.vertices)))
    mesh.fix_normals()
    os.makedirs(os.path.dirname(output_mesh_path) or ".", exist_ok=True)
    save_obj(output_mesh_path, mesh)
    logger.info("Mesh exported to: {}".format(output_mesh_path))
    shutil.rmtree(os.path.join(data_dir, "output"), ignore_errors=True)


def plan_device_postprocess(data_dir, max_steps, resolution, output_mesh_path, mesh_exe, simplify=None, report_views=False, texture=None, keep_seen=None, texture_from=None,
                            repair=None, report_topology=False, fill_holes=None, drop_intersecting=None, report_intersections=False, smooth=None, snap=None, report_residual=False):
    """The last stage on the device: one `build/mesh` process that extracts the mesh of the stage-2 snapshot (plan_two_stage passes --save-snapshot) at `resolution`,
    keeps the largest connected component and turns it outward (include/rnb_mesh_clean.h), and writes `output_mesh_path`. Pure; the snapshot named here is the first
    of snapshot_candidates, run_device_postprocess replaces it by the one that exists. simplify = N: the cleaned mesh is then simplified on N^3 cells over the
    scene's box (include/rnb_mesh_simplify.h, build/mesh --simplify N); None (the default) plans the command without it. report_views: the final mesh is also rasterised into
    every camera of the scene and compared with the input normal maps (include/rnb_mesh_raster.h, build/mesh --report-views writes <out>.views.json); False (the
    default) plans the command without it. texture = S: the final mesh also gets an albedo texture of S x S texels baked on the device (include/rnb_mesh_texture.h,
    build/mesh --texture S writes <out> with vt records, the .mtl and the _albedo.png beside it); None (the default) plans the command without it.
    keep_seen = "component" or "faces", or a dict(unit=..., min_views=N, rings=R, masks=True, max_off=N, supersample=K) of which only `unit` is needed: what no camera of
    the scene sees is dropped on the device after the cleaning and before the simplification (include/rnb_mesh_visibility.h, build/mesh --keep-seen ... and its
    --seen-* flags); None (the default) plans the command without it. texture_from = "views" (with texture only): the texture is projected from the scene's albedo maps
    through their cameras (include/rnb_mesh_project.h, build/mesh --texture-from views), the model's albedo where no view reaches; None (the default) plans the command without it.
    repair = True or a dict(weld=bool, duplicates="keep" / "first" / "cancel", orient_consistent=bool): the mesh is repaired on the device after the simplification, and
    the cleaning then acts on the repaired mesh (include/rnb_mesh_topology.h, build/mesh --repair and its flags); report_topology: build/mesh --report-topology prints
    the census of the final mesh as one JSON line. None / False (the defaults) plan the command without them.
    fill_holes = True or a dict(max_edges=N, skip_largest=bool): the boundary loops of the mesh are closed on the device after keep_seen, the simplification and the repair,
    and the cleaning then acts on the filled mesh (include/rnb_mesh_holes.h, build/mesh --fill-holes and its flags); None (the default) plans the command without it.
    drop_intersecting = "proper" or "all", or a dict(classes=..., rings=R): the triangles that pass through (all: or touch) other triangles of the mesh are removed on
    the device after the simplification and the repair and before fill_holes, which closes the rims (include/rnb_mesh_intersect.h, build/mesh --drop-intersecting and
    --drop-rings); report_intersections: build/mesh --report-intersections prints the self-intersection census of the final mesh as one JSON line. None / False (the
    defaults) plan the command without them.
    smooth = N or a dict(passes=N, lam=L, mu=M, boundary="pin" / "slide" / "free", only_fills=R, normals="keep" / "recompute") of which only `passes` is needed: the
    mesh is smoothed on the device by N passes over the one-ring right after fill_holes (include/rnb_mesh_smooth.h, build/mesh --smooth N and its --smooth-* flags);
    only_fills needs fill_holes. None (the default) plans the command without it.
    snap = N or a dict(iterations=N, tolerance=T, max_step=S, max_displacement=D, only_fills=bool, attributes="keep" / "resample") of which only `iterations` is needed:
    the vertices are moved back onto the model's surface on the device by up to N guarded Newton steps right after smooth (include/rnb_mesh_snap.h, build/mesh --snap N
    and its --snap-* flags); only_fills needs fill_holes. report_residual: build/mesh --report-residual prints mean and maximum |sdf| of the final mesh as one JSON
    line. None / False (the defaults) plan the command without them."""
    if texture_from is not None and texture is None:
        raise ValueError("texture_from needs texture")
    if texture_from not in (None, "views"):
        raise ValueError("texture_from must be 'views'")
    argv = [str(mesh_exe), "--snapshot", snapshot_candidates(data_dir, max_steps)[0], "--scene", str(data_dir), "--out", str(output_mesh_path),
            "--resolution", str(resolution), "--keep", "largest", "--orient", "outward"]
    if simplify is not None:
        argv += ["--simplify", str(int(simplify))]
    if report_views:
        argv += ["--report-views"]
    if texture is not None:
        argv += ["--texture", str(int(texture))]
    if texture_from is not None:
        argv += ["--texture-from", texture_from]
    if keep_seen is not None:
        argv += keep_seen_flags(keep_seen)
    if repair:
        argv += repair_flags(repair)
    if report_topology:
        argv += ["--report-topology"]
    if fill_holes:
        argv += fill_holes_flags(fill_holes)
    if drop_intersecting:
        argv += drop_intersecting_flags(drop_intersecting)
    if report_intersections:
        argv += ["--report-intersections"]
    if smooth is not None:
        argv += smooth_flags(smooth, fill_holes=bool(fill_holes))
    if snap is not None:
        argv += snap_flags(snap, fill_holes=bool(fill_holes))
    if report_residual:
        argv += ["--report-residual"]
    return argv


def smooth_flags(smooth, fill_holes=True):
    """The --smooth flags of build/mesh for plan_device_postprocess' smooth; fill_holes: whether the command also fills (only_fills needs it)."""
    sm = dict(passes=smooth) if isinstance(smooth, int) and not isinstance(smooth, bool) else (dict(smooth) if isinstance(smooth, dict) else None)
    if sm is None or set(sm) - {"passes", "lam", "mu", "boundary", "only_fills", "normals"} or sm.get("passes") is None or not 0 <= int(sm["passes"]) <= 10000:
        raise ValueError("smooth must be a number of passes (0 .. 10000) or a dict of passes and any of lam, mu, boundary, only_fills, normals")
    if sm.get("lam") is not None and not 0.0 < float(sm["lam"]) <= 1.0:
        raise ValueError("smooth: lam must be above 0 and at most 1")
    if sm.get("mu") is not None and not -1.5 <= float(sm["mu"]) <= 0.0:
        raise ValueError("smooth: mu must be at least -1.5 and at most 0")
    if sm.get("boundary") not in (None, "pin", "slide", "free"):
        raise ValueError("smooth: boundary must be 'pin', 'slide' or 'free'")
    if sm.get("normals") not in (None, "keep", "recompute"):
        raise ValueError("smooth: normals must be 'keep' or 'recompute'")
    if sm.get("only_fills") is not None and (not fill_holes or not 0 <= int(sm["only_fills"]) <= 1024):
        raise ValueError("smooth: only_fills (0 .. 1024) needs fill_holes")
    argv = ["--smooth", str(int(sm["passes"]))]
    for key, flag in (("lam", "--smooth-lambda"), ("mu", "--smooth-mu")):
        if sm.get(key) is not None:
            argv += [flag, repr(float(sm[key]))]
    if sm.get("boundary") is not None:
        argv += ["--smooth-boundary", sm["boundary"]]
    if sm.get("only_fills") is not None:
        argv += ["--smooth-only-fills", str(int(sm["only_fills"]))]
    if sm.get("normals") is not None:
        argv += ["--smooth-normals", sm["normals"]]
    return argv


def snap_flags(snap, fill_holes=True):
    """The --snap flags of build/mesh for plan_device_postprocess' snap; fill_holes: whether the command also fills (only_fills needs it)."""
    sn = dict(iterations=snap) if isinstance(snap, int) and not isinstance(snap, bool) else (dict(snap) if isinstance(snap, dict) else None)
    if sn is None or set(sn) - {"iterations", "tolerance", "max_step", "max_displacement", "only_fills", "attributes"} or sn.get("iterations") is None or not 0 <= int(sn["iterations"]) <= 64:
        raise ValueError("snap must be a number of iterations (0 .. 64) or a dict of iterations and any of tolerance, max_step, max_displacement, only_fills, attributes")
    for key, strict in (("tolerance", False), ("max_step", True), ("max_displacement", False)):
        if sn.get(key) is not None and not (0.0 < float(sn[key]) < float("inf") if strict else 0.0 <= float(sn[key]) < float("inf")):
            raise ValueError("snap: %s must be finite and %s 0" % (key, "above" if strict else "at least"))
    if sn.get("attributes") not in (None, "keep", "resample"):
        raise ValueError("snap: attributes must be 'keep' or 'resample'")
    if sn.get("only_fills") and not fill_holes:
        raise ValueError("snap: only_fills needs fill_holes")
    argv = ["--snap", str(int(sn["iterations"]))]
    for key, flag in (("tolerance", "--snap-tolerance"), ("max_step", "--snap-max-step"), ("max_displacement", "--snap-max-displacement")):
        if sn.get(key) is not None:
            argv += [flag, repr(float(sn[key]))]
    if sn.get("only_fills"):
        argv += ["--snap-only-fills"]
    if sn.get("attributes") is not None:
        argv += ["--snap-attributes", sn["attributes"]]
    return argv


def drop_intersecting_flags(drop_intersecting):
    """The --drop-intersecting flags of build/mesh for plan_device_postprocess' drop_intersecting."""
    di = dict(classes=drop_intersecting) if isinstance(drop_intersecting, str) else dict(drop_intersecting)
    if set(di) - {"classes", "rings"} or di.get("classes") not in ("proper", "all") or not 0 <= int(di.get("rings") or 0) <= 8:
        raise ValueError("drop_intersecting must be 'proper', 'all' or a dict of classes ('proper' / 'all') and rings (0 .. 8)")
    argv = ["--drop-intersecting", di["classes"]]
    if di.get("rings") is not None:
        argv += ["--drop-rings", str(int(di["rings"]))]
    return argv


def fill_holes_flags(fill_holes):
    """The --fill-holes flags of build/mesh for plan_device_postprocess' fill_holes."""
    fh = {} if fill_holes is True else dict(fill_holes)
    if set(fh) - {"max_edges", "skip_largest"} or (fh.get("max_edges") is not None and int(fh["max_edges"]) < 3):
        raise ValueError("fill_holes must be True or a dict of max_edges (at least 3) and skip_largest")
    argv = ["--fill-holes"]
    if fh.get("max_edges") is not None:
        argv += ["--fill-max-edges", str(int(fh["max_edges"]))]
    if fh.get("skip_largest"):
        argv += ["--fill-skip-largest"]
    return argv


def repair_flags(repair):
    """The --repair flags of build/mesh for plan_device_postprocess' repair."""
    rp = {} if repair is True else dict(repair)
    if set(rp) - {"weld", "duplicates", "orient_consistent"} or rp.get("duplicates") not in (None, "keep", "first", "cancel"):
        raise ValueError("repair must be True or a dict of weld, duplicates ('keep', 'first' or 'cancel') and orient_consistent")
    argv = ["--repair"]
    if rp.get("weld"):
        argv += ["--weld"]
    if rp.get("duplicates") is not None:
        argv += ["--duplicates", rp["duplicates"]]
    if rp.get("orient_consistent"):
        argv += ["--orient-consistent"]
    return argv


def keep_seen_flags(keep_seen):
    """The --keep-seen / --seen-* flags of build/mesh for plan_device_postprocess' keep_seen."""
    ks = dict(unit=keep_seen) if isinstance(keep_seen, str) else dict(keep_seen)
    unknown = set(ks) - {"unit", "min_views", "rings", "masks", "max_off", "supersample"}
    if unknown or ks.get("unit") not in ("component", "faces"):
        raise ValueError("keep_seen must be 'component', 'faces' or a dict with unit = one of them and any of min_views, rings, masks, max_off, supersample")
    if ks.get("rings") is not None and ks["unit"] != "faces":
        raise ValueError("keep_seen: rings needs unit = 'faces'")
    if ks.get("max_off") is not None and not ks.get("masks"):
        raise ValueError("keep_seen: max_off needs masks")
    argv = ["--keep-seen", ks["unit"]]
    for key, flag in (("min_views", "--seen-min-views"), ("rings", "--seen-rings")):
        if ks.get(key) is not None:
            argv += [flag, str(int(ks[key]))]
    if ks.get("masks"):
        argv += ["--seen-masks"]
        if ks.get("max_off") is not None:
            argv += ["--seen-max-off", str(int(ks["max_off"]))]
    if ks.get("supersample") is not None:
        argv += ["--seen-supersample", str(int(ks["supersample"]))]
    return argv


def default_mesh_exe(testbed_path):
    """build/mesh beside build/testbed."""
    return os.path.join(os.path.dirname(os.path.abspath(testbed_path)), "mesh")


def run_device_postprocess(data_dir, max_steps, resolution, output_mesh_path, mesh_exe, logger=None, simplify=None, report_views=False, texture=None, keep_seen=None,
                           texture_from=None, repair=None, report_topology=False, fill_holes=None, drop_intersecting=None, report_intersections=False, smooth=None, snap=None,
                           report_residual=False):
    """postprocess_mesh's job without the OBJ round trip: runs plan_device_postprocess' command, then drops the training output directory as postprocess_mesh does."""
    logger = logger or SimpleLogger()
    cmd = plan_device_postprocess(data_dir, max_steps, resolution, output_mesh_path, mesh_exe, simplify=simplify, report_views=report_views, texture=texture, keep_seen=keep_seen,
                                  texture_from=texture_from, repair=repair, report_topology=report_topology, fill_holes=fill_holes,
                                  drop_intersecting=drop_intersecting, report_intersections=report_intersections, smooth=smooth, snap=snap, report_residual=report_residual)
    found = [p for p in snapshot_candidates(data_dir, max_steps) if os.path.exists(p)]
    if not found:
        raise RuntimeError("Snapshot not found after {} iterations".format(max_steps))
    cmd[cmd.index("--snapshot") + 1] = found[0]
    os.makedirs(os.path.dirname(output_mesh_path) or ".", exist_ok=True)
    logger.info("Post-processing on the device: {}".format(" ".join(cmd)))
    result = subprocess.run(cmd, capture_output=True, text=True)
    if result.stdout:
        for line in result.stdout.strip().split("\n"):
            logger.info(line)
    if result.returncode != 0:
        if result.stderr:
            logger.error(result.stderr)
        raise RuntimeError("Device post-processing failed with code {}".format(result.returncode))
    logger.info("Mesh exported to: {}".format(output_mesh_path))
    shutil.rmtree(os.path.join(data_dir, "output"), ignore_errors=True)


def run_full_pipeline(input_path, testbed_path, output_dir, max_steps=10000, mesh_resolution=1024, scaling_mode="auto", sphere_scale=1.0, margin_px=20,
                      warmup_ratio=0.1, mask_weight=1.0, super_normal=False, use_l1=False, use_rgb_plus=True, has_albedo=False,
                      albedo_sfm_path="", mask_sfm_path="", mask_folder_path="", n_samples=2000, logger=None, device_postprocess=False, mesh_exe=None, simplify=None, report_views=False, texture=None,
                      keep_seen=None, texture_from=None, repair=None, report_topology=False, fill_holes=None, drop_intersecting=None, report_intersections=False, smooth=None, snap=None,
                      report_residual=False):
    """load -> prepare (<output_dir>/prepared_data) -> train (two-stage, or warm-up + albedo scaling + two-stage when
    `has_albedo`) -> post-process to <output_dir>/mesh.obj, which is returned. (pipeline.py:222-305)
    device_postprocess: the last step runs on the GPU (run_device_postprocess; mesh_exe defaults to build/mesh beside the testbed) instead of postprocess_mesh;
    simplify = N (with device_postprocess only): that step also simplifies the mesh on N^3 cells (build/mesh --simplify N);
    report_views (with device_postprocess only): that step also writes <output_dir>/mesh.obj.views.json, the mesh's normal angle and mask IoU per input view (with texture as well:
    the textured mesh's, textured_* and albedo_* of include/rnb_mesh_draw.h, whose lines build/mesh prints and this function logs with the others);
    texture = S (with device_postprocess only): that step also bakes an albedo texture of S x S texels: mesh.obj gets vt records, mesh.mtl and mesh_albedo.png beside it;
    keep_seen (with device_postprocess only): that step also drops what no camera sees (plan_device_postprocess describes the value; build/mesh --keep-seen);
    texture_from = "views" (with texture only): the texture is projected from the input albedo maps instead of baked from the model (build/mesh --texture-from views);
    repair / report_topology (with device_postprocess only): that step also repairs the mesh after the simplification / prints its census (plan_device_postprocess
    describes the values; build/mesh --repair, --report-topology);
    fill_holes (with device_postprocess only): that step also closes the boundary loops of the mesh (plan_device_postprocess describes the value; build/mesh --fill-holes).
    drop_intersecting, report_intersections (with device_postprocess only): that step also removes the self-intersecting triangles before it fills, and prints the
    self-intersection census of the final mesh (plan_device_postprocess describes the values; build/mesh --drop-intersecting, --report-intersections).
    smooth (with device_postprocess only): that step also smooths the mesh after it fills (plan_device_postprocess describes the value; build/mesh --smooth).
    snap, report_residual (with device_postprocess only): that step also moves the vertices back onto the model's surface after it smooths, and prints mean and maximum
    |sdf| of the final mesh (plan_device_postprocess describes the values; build/mesh --snap, --report-residual)."""
    if (snap is not None or report_residual) and not device_postprocess:
        raise ValueError("snap and report_residual need device_postprocess")
    if smooth is not None and not device_postprocess:
        raise ValueError("smooth needs device_postprocess")
    if (repair or report_topology) and not device_postprocess:
        raise ValueError("repair and report_topology need device_postprocess")
    if fill_holes and not device_postprocess:
        raise ValueError("fill_holes needs device_postprocess")
    if (drop_intersecting or report_intersections) and not device_postprocess:
        raise ValueError("drop_intersecting and report_intersections need device_postprocess")
    if texture_from is not None and texture is None:
        raise ValueError("texture_from needs texture")
    if keep_seen is not None and not device_postprocess:
        raise ValueError("keep_seen needs device_postprocess")
    if simplify is not None and not device_postprocess:
        raise ValueError("simplify needs device_postprocess")
    if report_views and not device_postprocess:
        raise ValueError("report_views needs device_postprocess")
    if texture is not None and not device_postprocess:
        raise ValueError("texture needs device_postprocess")
    logger = logger or SimpleLogger()
    from .dataloaders import load_data
    from .prepare import prepare_testbed_data

    logger.info("=== Loading data from {} ===".format(input_path))
    data = load_data(input_path, albedo_sfm_path=albedo_sfm_path, mask_sfm_path=mask_sfm_path, mask_folder_path=mask_folder_path, logger=logger)
    data_dir = os.path.join(output_dir, "prepared_data")
    logger.info("=== Preparing testbed data ===")
    prepare_testbed_data(data, data_dir, logger, scaling_mode=scaling_mode, sphere_scale=sphere_scale, margin_px=margin_px)
    flags = common_flags(mask_weight, super_normal, use_l1, use_rgb_plus)
    if has_albedo:
        run_with_albedo_scaling(testbed_path, data_dir, max_steps, flags, resolution=mesh_resolution, warmup_ratio=warmup_ratio, n_samples=n_samples, logger=logger)
    else:
        run_two_stage(testbed_path, data_dir, max_steps, flags, resolution=mesh_resolution, no_albedo=True, logger=logger)
    output_mesh = os.path.join(output_dir, "mesh.obj")
    if device_postprocess:
        run_device_postprocess(data_dir, max_steps, mesh_resolution, output_mesh, mesh_exe or default_mesh_exe(testbed_path), logger, simplify=simplify, report_views=report_views, texture=texture,
                               keep_seen=keep_seen, texture_from=texture_from, repair=repair, report_topology=report_topology, fill_holes=fill_holes,
                               drop_intersecting=drop_intersecting, report_intersections=report_intersections, smooth=smooth, snap=snap, report_residual=report_residual)
    else:
        postprocess_mesh(data_dir, output_mesh, logger)
    logger.info("=== Pipeline complete ===")
    return output_mesh
