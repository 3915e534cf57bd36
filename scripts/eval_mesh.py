#!/usr/bin/env python
"""Mesh reconstruction metrics of the meshes scripts/eval.py writes against the ground-truth STLs
they were meant to reconstruct (map), then their means over all objects (reduce).  The reference has
no counterpart: its eval/eval.py stops at the STL.

  python scripts/eval_mesh.py -O <eval output> -G <ground-truth dir> [--mesh_res 256] \
      [--normalize both|gt|none] [--gt_radius 1.0] [--n_samples 100000] [--tau 0.01] [--seed 0] \
      [--iou] [--n_iou_points 100000] [--components all|largest] [--min_component_frac F] \
      [--sil_views N] [--sil_size 128] [--sil_focal 131.25] \
      [--metrics_backend auto|hip|numpy] [--overwrite] [-R]

Map: every folder ``<object>`` of the output root that holds ``<object>_mesh.stl`` is paired with
``<ground-truth dir>/<object>.stl``; a missing ground truth skips the object with one line on
stderr.  eval.py writes vertices in grid index units: they are mapped to the grid's world cube
[-1, 1]^3 with ``v * 2 / (mesh_res - 1) - 1``.  --normalize both (the default) then brings each mesh
to the unit sphere by its own bounds (pnr.mesh.normalize_bounds: bounding-box centre to the origin,
farthest vertex to radius 1), the scale the usual tau = 0.01 is meant for; ``gt`` transforms only the
ground truth, to --gt_radius (what the fork's Blender step does before it renders the views);
``none`` compares the two as they stand.  pnr.evaluate.mesh_metrics scores the pair (on the device
with the hip backend) and ``<object>/mesh_metrics.txt`` gets one ``name value`` line per score.

Reduce: every folder of the output root whose name does not start with "_" and that holds a
``mesh_metrics.txt`` contributes it; ``all_mesh_metrics.txt`` gets one ``name mean`` line per score
and a last line ``objects N``.

--iou adds the volumetric IoU (pnr.evaluate.volume_iou: --n_iou_points uniform points in the padded
bounds of the pair as it is scored, drawn with --seed, each classified by its generalized winding
number against each mesh): ``mesh_metrics.txt`` gets the lines ``iou``, ``volume_pred``,
``volume_gt`` and ``n_points`` after the others, and the reduce averages them too.  A contributing
file without them (written by a run without --iou) stops the reduce with the object's name.  Without
--iou both files are what they were.

--components largest, or --min_component_frac F (0 < F <= 1; not both), cleans the PREDICTED mesh
before it is scored (pnr.evaluate.clean_mesh; the ground truth is left as it is): the STL's soup is
welded, its connected components are labelled, and only the component with the most faces, or every
component with at least F times the faces of the largest, is kept.  This happens on the index-unit
vertices, before they are mapped to the world cube and normalised, so a floater no longer moves the
bounds the prediction is normalised by.  ``mesh_metrics.txt`` then ends with the lines
``n_components``, ``n_components_kept`` and ``faces_kept``, and the reduce averages them; as with
--iou, a contributing file without them stops the reduce with the object's name.  With both flags
at their defaults every file is what it was.

--sil_views N (default 0: off) adds the 2D scores of single-view reconstruction work
(pnr.evaluate.silhouette_scores; pnr.ops.mesh_raster, csrc/meshraster.hip, with the hip backend): the
pair as it is scored, after normalisation and cleanup, is rendered from the N cameras of
pnr.evaluate.sphere_poses at --sil_size pixels with the focal length --sil_focal, at the radius from
which a sphere of radius 1.05 fills that field of view (so a pair normalised to the unit sphere is
seen whole).  ``mesh_metrics.txt`` then ends with the lines ``sil_iou`` (the mean silhouette IoU
over the views), ``sil_depth_l1`` (the mean depth difference over the pixels both meshes cover) and
``sil_views``, and the reduce averages them; a contributing file without them stops the reduce with
the object's name.  With the default every file is byte for byte what it was.
"""
import argparse
import os
import os.path as osp
import sys

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.join(REPO, "pixel-nerf_amd"))

OUT_NAME = "mesh_metrics.txt"


def add_mesh_metric_args(ap):
    """The flags scripts/eval.py --gt_mesh_dir shares with this script."""
    ap.add_argument("--normalize", choices=("both", "gt", "none"), default="both",
                    help="both = each mesh to the unit sphere by its own bounds; gt = only the ground truth, to "
                         "--gt_radius; none = as they stand")
    ap.add_argument("--gt_radius", type=float, default=1.0, help="radius of --normalize gt")
    ap.add_argument("--n_samples", type=int, default=100000, help="surface samples per mesh")
    ap.add_argument("--tau", type=float, default=0.01, help="distance threshold of precision / recall / F-score")
    ap.add_argument("--seed", type=int, default=0, help="seed of the surface samples (and of the --iou points)")
    ap.add_argument("--iou", action="store_true",
                    help="also score the volumetric IoU (winding-number containment) into mesh_metrics.txt")
    ap.add_argument("--n_iou_points", type=int, default=100000, help="uniform points of --iou")
    ap.add_argument("--components", choices=("all", "largest"), default="all",
                    help="largest = score only the predicted mesh's connected component with the most faces "
                         "(welded first); all = every component")
    ap.add_argument("--min_component_frac", type=float, default=None, metavar="F",
                    help="keep the predicted mesh's components with at least F x the faces of the largest "
                         "(0 < F <= 1; not with --components largest)")
    ap.add_argument("--sil_views", type=int, default=0, metavar="N",
                    help="also score the silhouette IoU and depth error from N cameras around the pair (0 = off)")
    ap.add_argument("--sil_size", type=int, default=128, help="image side of --sil_views, pixels")
    ap.add_argument("--sil_focal", type=float, default=131.25, help="focal length of --sil_views, pixels")


def component_args_error(args):
    """The message for a bad combination of the cleanup flags, or None."""
    if args.min_component_frac is not None:
        if args.components == "largest":
            return "--min_component_frac goes with --components all (largest keeps one component)"
        if not 0.0 < args.min_component_frac <= 1.0:
            return "--min_component_frac must be in (0, 1]"
    return None


def sil_args_error(args):
    """The message for bad silhouette flags, or None."""
    if args.sil_views < 0:
        return "--sil_views must be >= 0"
    if args.sil_views and (args.sil_size < 1 or not args.sil_focal > 0.0):
        return "--sil_size must be >= 1 and --sil_focal > 0"
    return None


def sil_radius(args):
    """The camera distance from which a sphere of radius 1.05 at the origin fills the field of view."""
    import math

    return 1.05 / math.sin(math.atan(0.5 * args.sil_size / args.sil_focal))


def silhouette(pred, gt, args, backend):
    """pnr.evaluate.silhouette_scores of the pair from the --sil_views cameras."""
    import torch

    from pnr import evaluate

    poses, _ = evaluate.sphere_poses(args.sil_views, sil_radius(args))
    return evaluate.silhouette_scores(pred, gt, torch.from_numpy(poses).float(), args.sil_size, args.sil_size,
                                      args.sil_focal, backend=backend)


def cleaning(args):
    """Whether the predicted mesh is cleaned before it is scored."""
    return args.components == "largest" or args.min_component_frac is not None


def clean_pred(verts, faces, args, backend):
    """The predicted mesh (index units) with its floaters dropped as the flags ask: (verts, faces,
    info) of pnr.evaluate.clean_mesh on `backend`."""
    from pnr import evaluate

    return evaluate.clean_mesh(verts, faces, weld=True, keep=args.components, min_frac=args.min_component_frac,
                               by="faces", backend=backend)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Chamfer / F-score / normal consistency / IoU of extracted meshes.")
    ap.add_argument("--output", "-O", type=str, default="eval", help="Root path of the eval.py output")
    ap.add_argument("--gt_mesh_dir", "-G", type=str, required=True, help="ground truth, <object>.stl")
    ap.add_argument("--mesh_res", type=int, default=256, help="the --mesh_res eval.py ran with")
    add_mesh_metric_args(ap)
    ap.add_argument("--metrics_backend", choices=("auto", "hip", "numpy"), default="auto",
                    help="hip = sample and search on the device (pnr.ops), numpy = on the host; auto = hip when a "
                         "HIP device is present, else numpy")
    ap.add_argument("--gpu_id", type=int, default=0, help="GPU id (hip backend)")
    ap.add_argument("--overwrite", action="store_true", help="overwrite existing mesh_metrics.txt")
    ap.add_argument("--reduce_only", "-R", action="store_true", help="skip the map (per-object metrics)")
    return ap.parse_args(argv)


def grid_to_world(verts, mesh_res):
    """eval.py's index-unit vertices on the mesh_res^3 grid over [-1, 1]^3."""
    return verts * (2.0 / (mesh_res - 1)) - 1.0


def prepare_pair(pred_verts, gt_verts, args):
    """The two vertex sets as they are scored (arrays or tensors; the predicted one in world units)."""
    from pnr import mesh

    if args.normalize == "both":
        return mesh.normalize_bounds(pred_verts), mesh.normalize_bounds(gt_verts)
    if args.normalize == "gt":
        return pred_verts, mesh.normalize_bounds(gt_verts, args.gt_radius)
    return pred_verts, gt_verts


def metric_names(args):
    """The lines of a metrics file, in order: the surface scores, then with --iou the volume scores,
    then with a cleanup flag the component counts, then with --sil_views the silhouette scores."""
    from pnr import evaluate

    return (tuple(evaluate.MESH_METRIC_NAMES) + (tuple(evaluate.VOLUME_METRIC_NAMES) if args.iou else ())
            + (tuple(evaluate.CLEAN_INFO_NAMES) if cleaning(args) else ())
            + (tuple(evaluate.SIL_METRIC_NAMES) if args.sil_views else ()))


def write_metrics(path, scores, names):
    with open(path, "w") as f:
        f.write("".join("{} {!r}\n".format(k, float(scores[k])) for k in names))


def score_object(pred, gt_path, out_path, args, backend, clean_info=None):
    """pred = (verts in world units, faces), already cleaned when a cleanup flag is set (clean_info:
    clean_pred's info, whose counts then follow the scores); writes out_path, returns the scores."""
    from pnr import evaluate, mesh

    gv, gf = mesh.read_stl_indexed(gt_path)
    pv, gv = prepare_pair(pred[0], gv, args)
    scores = evaluate.mesh_metrics((pv, pred[1]), (gv, gf), n_samples=args.n_samples, tau=args.tau, seed=args.seed,
                                   backend=backend)
    if args.iou:
        scores.update(evaluate.volume_iou((pv, pred[1]), (gv, gf), n_points=args.n_iou_points, seed=args.seed,
                                          backend=backend))
    if cleaning(args):
        scores.update(clean_info)
    if args.sil_views:
        scores.update(silhouette((pv, pred[1]), (gv, gf), args, backend))
    write_metrics(out_path, scores, metric_names(args))
    return scores


def resolve_backend(args):
    from pnr import evaluate

    backend = evaluate._resolve_backend(args.metrics_backend, "metrics")
    if backend == "hip":
        import torch

        torch.cuda.set_device(args.gpu_id)
    return backend


def run_map(args):
    from pnr import mesh

    backend = resolve_backend(args)
    print("Scoring with the", backend, "backend")
    done = 0
    for name in sorted(os.listdir(args.output)):
        stl = osp.join(args.output, name, name + "_mesh.stl")
        if name[0] == "_" or not osp.isfile(stl):
            continue
        out_path = osp.join(args.output, name, OUT_NAME)
        if osp.exists(out_path) and not args.overwrite:
            continue
        gt_path = osp.join(args.gt_mesh_dir, name + ".stl")
        if not osp.isfile(gt_path):
            print("eval_mesh: no ground truth %s; %s skipped" % (gt_path, name), file=sys.stderr)
            continue
        pv, pf = mesh.read_stl_indexed(stl)
        info = None
        if cleaning(args):   # on the index-unit soup, before the world map and the normalisation
            pv, pf, info = clean_pred(pv, pf, args, backend)
        score_object((grid_to_world(pv, args.mesh_res), pf), gt_path, out_path, args, backend, clean_info=info)
        done += 1
    print(">>> SCORED", done, "OBJECTS")


def read_metrics(path):
    with open(path, "r") as f:
        return {tok[0]: float(tok[1]) for tok in (line.split() for line in f) if len(tok) == 2}


def run_reduce(args):
    folders = sorted(x for x in os.listdir(args.output)
                     if x[0] != "_" and osp.isfile(osp.join(args.output, x, OUT_NAME)))
    print(">>> PROCESSING", len(folders), "OBJECTS")
    if not folders:
        raise SystemExit("eval_mesh: no %s under %s" % (OUT_NAME, args.output))
    rows = [read_metrics(osp.join(args.output, x, OUT_NAME)) for x in folders]
    from pnr import evaluate

    names = metric_names(args)
    if args.iou:
        for x, row in zip(folders, rows):
            if any(name not in row for name in evaluate.VOLUME_METRIC_NAMES):
                raise SystemExit("eval_mesh: %s of object %s has no volume scores (scored without --iou; run the map "
                                 "again with --iou --overwrite)" % (OUT_NAME, x))
    if cleaning(args):
        for x, row in zip(folders, rows):
            if any(name not in row for name in evaluate.CLEAN_INFO_NAMES):
                raise SystemExit("eval_mesh: %s of object %s has no component counts (scored without --components / "
                                 "--min_component_frac; run the map again with the flag and --overwrite)"
                                 % (OUT_NAME, x))
    if args.sil_views:
        for x, row in zip(folders, rows):
            if any(name not in row for name in evaluate.SIL_METRIC_NAMES):
                raise SystemExit("eval_mesh: %s of object %s has no silhouette scores (scored without --sil_views; run "
                                 "the map again with --sil_views and --overwrite)" % (OUT_NAME, x))
    lines = []
    for name in names:
        acc = 0.0
        for row in rows:   # in order from 0.0, divided once
            acc += row[name]
        lines.append("{} {!r}".format(name, acc / len(rows)))
    lines.append("objects {}".format(len(rows)))
    out_path = osp.join(args.output, "all_mesh_metrics.txt")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("WROTE", out_path)
    print("\n".join(lines))


def main(argv=None):
    args = parse_args(argv)
    if args.mesh_res < 2:
        raise SystemExit("eval_mesh: --mesh_res must be >= 2")
    if args.n_iou_points < 1:
        raise SystemExit("eval_mesh: --n_iou_points must be >= 1")
    if component_args_error(args):
        raise SystemExit("eval_mesh: " + component_args_error(args))
    if sil_args_error(args):
        raise SystemExit("eval_mesh: " + sil_args_error(args))
    if not args.reduce_only:
        print(">>> Compute")
        run_map(args)
    print(">>> Reduce")
    run_reduce(args)


if __name__ == "__main__":
    main()
