#!/usr/bin/env python
"""eval/eval.py counterpart on the MI355X ray march: per object of an SRN-layout split, encode
the source views, query the density on a mesh_res^3 grid over [-1, 1]^3 (PixelNeRFNet.forward as
a point query, coarse net, zero view directions, 65,536-point chunks: eval.py:93-103), and
write the grid; with --compare, render every non-source view and score it (PSNR / SSIM,
skimage's compare_* defaults as pnr.evaluate restates them) into <output>/finish.txt as
"<object> <psnr> <ssim> 1" (eval.py:110-144).

  python scripts/eval.py -c conf/exp/srn.conf -D <datadir>/cars -n srn_car \
      --checkpoints_path checkpoints [--split test] [-P "2"] [--mesh_res 256] [--compare]

The reference turns the grid into a mesh with skimage.measure.marching_cubes and trimesh
(eval.py:104-108) and writes <output>/<object>/<object>_mesh.stl.  --mesh_backend picks the
extractor: `hip` runs pnr.ops.marching_cubes (csrc/mcubes.hip) on the grid while it is still on the
device and writes the binary STL with pnr.mesh; `skimage` is the reference's route; `auto` (the
default) is skimage where skimage and trimesh import and the device path otherwise.  A threshold
outside the grid's range gives a valid empty STL on the device path.  The grid is also written as
<output>/<object>/<object>_sigma.npy (float32, relu(sigma), [x][y][z] with torch.meshgrid's 'ij'
order).  In the fork the comparison after the mesh is unreachable (a `continue` follows the
export); --compare runs it, and --metrics_backend hip scores its views on the device
(pnr.ops.image_metrics, csrc/metrics.hip) instead of copying them to the host for numpy / scipy.

--gt_mesh_dir DIR (opt-in; the hip mesh backend only) scores each extracted mesh against
DIR/<object>.stl while its vertices and faces are still on the device (pnr.evaluate.mesh_metrics:
Chamfer-L1 / L2, accuracy / completeness, F-score, normal consistency) and writes
<output>/<object>/mesh_metrics.txt, the file scripts/eval_mesh.py writes from the STL, with that
script's --normalize / --gt_radius / --n_samples / --tau / --seed.  With --iou (and --n_iou_points)
the volumetric IoU (pnr.evaluate.volume_iou: winding-number containment, pnr.ops.mesh_contains,
csrc/winding.hip) is scored from the same device tensors and its lines follow in that file.  An
object without a ground-truth file is skipped with one line on stderr.  --components largest or
--min_component_frac F (scripts/eval_mesh.py's flags) drop the floaters of the device mesh before it
is scored (pnr.evaluate.clean_mesh: pnr.ops.mesh_weld / mesh_components / mesh_component_stats,
csrc/meshclean.hip) and add the component counts to mesh_metrics.txt; --write_clean_mesh also writes
the cleaned mesh as <output>/<object>/<object>_mesh_clean.stl beside the untouched
<object>_mesh.stl.  --sil_views N (with --sil_size / --sil_focal; scripts/eval_mesh.py's flags, off by
default) renders the pair as it is scored from N cameras around it (pnr.evaluate.silhouette_scores:
pnr.ops.mesh_raster, csrc/meshraster.hip) and ends mesh_metrics.txt with sil_iou, sil_depth_l1 and
sil_views."""
import argparse
import os
import sys
import time
import traceback

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "pixel-nerf_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))   # eval_mesh, also when this file is loaded by path

import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_mesh  # noqa: E402
from pnr import evaluate, mesh, ops, util  # noqa: E402
from pnr.conf import parse_file  # noqa: E402
from pnr.data import get_split_dataset  # noqa: E402
from pnr.models import PRECISIONS, make_model  # noqa: E402
from pnr.renderer import NeRFRenderer  # noqa: E402

CHUNK = 65536   # eval.py:99


def density_grid(net, res, device, chunk=CHUNK):
    """relu(sigma) of the coarse net on a res^3 grid over [-1, 1]^3 ('ij' order), (res, res, res)."""
    grid = torch.linspace(-1, 1, res, device=device)
    xs, ys, zs = torch.meshgrid(grid, grid, grid, indexing="ij")
    pts = torch.stack([xs, ys, zs], -1).reshape(-1, 3)
    out = torch.empty(pts.shape[0], device=device)
    with torch.no_grad():
        for i in range(0, pts.shape[0], chunk):
            p = pts[i:i + chunk][None]
            out[i:i + chunk] = net(p, coarse=True, viewdirs=torch.zeros_like(p))[0, :, 3]
    return torch.relu(out).view(res, res, res)


def _have_skimage():
    try:
        import skimage.measure  # noqa: F401
        import trimesh  # noqa: F401
    except ImportError:
        return False
    return True


def export_mesh(sig, thresh, path, backend="auto", keep=None):
    """The reference's mesh export (eval.py:104-108) of the grid `sig` (a device tensor, or a numpy
    array) to a binary STL at `path`.  Returns (backend used, triangles written, seconds spent
    extracting).  `hip`: pnr.ops.marching_cubes on the device grid + pnr.mesh.write_stl (an empty
    surface writes an empty STL); `skimage`: skimage + trimesh; `auto`: skimage where both import,
    else hip.  `keep`: a dict that receives the device path's "verts" / "faces" tensors."""
    if backend == "auto":
        backend = "skimage" if _have_skimage() else "hip"
    if backend == "skimage":
        import skimage.measure
        import trimesh

        sig_np = sig.cpu().numpy() if torch.is_tensor(sig) else sig
        t0 = time.perf_counter()
        verts, faces, _, _ = skimage.measure.marching_cubes(sig_np, level=thresh)
        dt = time.perf_counter() - t0
        trimesh.Trimesh(vertices=verts, faces=faces).export(path)
        return backend, int(len(faces)), dt
    if backend != "hip":
        raise ValueError("mesh backend %r (auto, hip, skimage)" % (backend,))
    if not torch.is_tensor(sig):
        sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float32)).cuda()
    torch.cuda.synchronize(sig.device)
    t0 = time.perf_counter()
    verts, faces = ops.marching_cubes(sig, thresh)
    torch.cuda.synchronize(sig.device)
    dt = time.perf_counter() - t0
    mesh.write_stl(path, verts, faces)
    if keep is not None:
        keep["verts"], keep["faces"] = verts, faces
    return backend, int(faces.shape[0]), dt


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--conf", "-c", required=True)
    ap.add_argument("--datadir", "-D", required=True)
    ap.add_argument("--dataset_format", "-F", default="srn")
    ap.add_argument("--name", "-n", default="srn_car")
    ap.add_argument("--checkpoints_path", default="checkpoints")
    ap.add_argument("--split", default="test")
    ap.add_argument("--source", "-P", default="2")
    ap.add_argument("--coarse", action="store_true")
    ap.add_argument("--output", "-O", default="eval")
    ap.add_argument("--mesh_res", type=int, default=256)
    ap.add_argument("--mesh_thresh", type=float, default=0.1)
    ap.add_argument("--mesh_backend", choices=("auto", "hip", "skimage"), default="auto",
                    help="isosurface extractor: hip = the device kernels, skimage = the reference's libraries, "
                         "auto = skimage where skimage and trimesh import, else hip")
    ap.add_argument("--compare", action="store_true", help="render and score the non-source views")
    ap.add_argument("--metrics_backend", choices=("numpy", "hip"), default="numpy",
                    help="where --compare scores the views: numpy = on the host, image by image; hip = on the "
                         "device (pnr.ops.image_metrics)")
    ap.add_argument("--gt_mesh_dir", default=None,
                    help="ground-truth meshes <object>.stl: score each extracted mesh on the device (needs the "
                         "hip mesh backend) into <object>/mesh_metrics.txt")
    eval_mesh.add_mesh_metric_args(ap)
    ap.add_argument("--write_clean_mesh", action="store_true",
                    help="with --components largest / --min_component_frac: also write <object>_mesh_clean.stl")
    ap.add_argument("--ray_batch_size", "-R", type=int, default=50000)
    ap.add_argument("--gpu_id", type=int, default=0)
    ap.add_argument("--precision", choices=sorted(PRECISIONS), default="f16x3",
                    help="arithmetic of the fused MLP (pnr.models.PRECISIONS); f16 trades accuracy below an "
                         "8-bit step for time")
    args = ap.parse_args(argv)
    args.resume = True
    if args.gt_mesh_dir is not None and args.mesh_backend == "skimage":
        ap.error("--gt_mesh_dir scores the device mesh: it needs --mesh_backend hip (or auto without skimage)")
    if eval_mesh.component_args_error(args):
        ap.error(eval_mesh.component_args_error(args))
    if eval_mesh.sil_args_error(args):
        ap.error(eval_mesh.sil_args_error(args))
    if args.write_clean_mesh and not eval_mesh.cleaning(args):
        ap.error("--write_clean_mesh needs --components largest or --min_component_frac")
    if args.write_clean_mesh and args.mesh_backend == "skimage":
        ap.error("--write_clean_mesh cleans the device mesh: it needs --mesh_backend hip (or auto without skimage)")

    device = torch.device("cuda", args.gpu_id)
    torch.cuda.set_device(device)
    conf = parse_file(args.conf)
    dset = get_split_dataset(args.dataset_format, args.datadir, want_split=args.split, training=False)
    net = make_model(conf["model"]).to(device=device).load_weights(args)
    net.mlp_precision = args.precision
    net.eval()
    renderer = NeRFRenderer.from_conf(conf["renderer"], lindisp=dset.lindisp,
                                      eval_batch_size=args.ray_batch_size).to(device)
    if args.coarse:
        net.mlp_fine = None
    renderer.n_coarse = max(renderer.n_coarse, 64)
    render_par = renderer.bind_parallel(net, None, simple_output=True).eval()
    source = torch.tensor(sorted(map(int, args.source.split())), dtype=torch.long)
    os.makedirs(args.output, exist_ok=True)
    finish = open(os.path.join(args.output, "finish.txt"), "a", buffering=1)
    for obj_idx in range(len(dset)):
        name = str(obj_idx)
        try:
            data = dset[obj_idx]
            name = os.path.basename(data["path"])
            out_dir = os.path.join(args.output, name)
            os.makedirs(out_dir, exist_ok=True)
            images, poses = data["images"], data["poses"]
            if images.shape[0] < 2:
                print("Skipping %s - less than 2 views" % name, flush=True)
                continue
            focal = torch.as_tensor(data["focal"], dtype=torch.float32)[None].to(device)
            c = data.get("c")
            c = c.to(device).unsqueeze(0) if c is not None else None
            src = torch.zeros(images.shape[0], dtype=torch.bool)
            src[source] = True
            with torch.no_grad():
                net.encode(images[src].to(device).unsqueeze(0), poses[src].to(device).unsqueeze(0), focal, c=c)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            sig = density_grid(net, args.mesh_res, device)
            torch.cuda.synchronize(device)
            dt = time.perf_counter() - t0
            # the device extractor reads the grid tensor where it is, before the host copy
            kept = {}
            backend, n_tri, dt_mesh = export_mesh(sig, args.mesh_thresh, os.path.join(out_dir, name + "_mesh.stl"),
                                                  args.mesh_backend, keep=kept)
            np.save(os.path.join(out_dir, name + "_sigma.npy"), sig.cpu().numpy())
            print("%s: density grid %d^3 in %.3f s (%.1f M points/s); mesh (%s) %d triangles in %.4f s%s" % (
                name, args.mesh_res, dt, args.mesh_res ** 3 / dt / 1e6, backend, n_tri, dt_mesh,
                "" if n_tri else ": threshold %g is outside the grid's range, empty STL written" % args.mesh_thresh),
                flush=True)
            clean_info = None
            wanted = args.gt_mesh_dir is not None or args.write_clean_mesh
            if backend == "hip" and eval_mesh.cleaning(args) and wanted:
                kept["verts"], kept["faces"], clean_info = eval_mesh.clean_pred(kept["verts"], kept["faces"], args,
                                                                                 "hip")
                print("%s: kept %d of %d components, %d of %d triangles" % (
                    name, clean_info["n_components_kept"], clean_info["n_components"], clean_info["faces_kept"],
                    n_tri), flush=True)
                if args.write_clean_mesh:
                    mesh.write_stl(os.path.join(out_dir, name + "_mesh_clean.stl"), kept["verts"], kept["faces"])
            if args.gt_mesh_dir is not None and backend != "hip":
                print("eval: --gt_mesh_dir needs the hip mesh backend (auto chose %s); mesh metrics of %s skipped"
                      % (backend, name), file=sys.stderr)
            elif args.gt_mesh_dir is not None:
                gt_path = os.path.join(args.gt_mesh_dir, name + ".stl")
                if not os.path.isfile(gt_path):
                    print("eval: no ground truth %s; mesh metrics of %s skipped" % (gt_path, name), file=sys.stderr)
                else:   # the device tensors, never the STL just written
                    pred = (eval_mesh.grid_to_world(kept["verts"], args.mesh_res), kept["faces"])
                    scores = eval_mesh.score_object(pred, gt_path, os.path.join(out_dir, eval_mesh.OUT_NAME), args,
                                                    "hip", clean_info=clean_info)
                    print("%s: chamfer_l1 %.6g fscore %.4f normal_consistency %.4f%s" % (
                        name, scores["chamfer_l1"], scores["fscore"], scores["normal_consistency"],
                        " iou %.4f" % scores["iou"] if args.iou else ""), flush=True)
            if not args.compare:
                continue
            tgt = ~src
            H, W = images.shape[-2:]
            rays = util.gen_rays(poses[tgt].to(device), W, H, focal, dset.z_near, dset.z_far, c=c).reshape(-1, 8)
            with torch.no_grad():
                rgb = torch.cat([render_par(r[None])[0][0] for r in torch.split(rays, args.ray_batch_size, dim=0)])
            gt = (images[tgt] * 0.5 + 0.5).permute(0, 2, 3, 1)
            if args.metrics_backend == "numpy":
                rgb = rgb.clamp(0.0, 1.0).reshape(-1, H, W, 3).cpu().numpy()
                gt = gt.numpy()
                psnr = float(np.mean([evaluate.psnr_np(rgb[i], gt[i]) for i in range(len(gt))]))
                ssim = float(np.mean([evaluate.ssim(rgb[i], gt[i]) for i in range(len(gt))]))
            else:   # all views of the object in one call, on the device the render is on
                psnrs, ssims = evaluate.image_metrics(rgb.clamp(0.0, 1.0).reshape(-1, H, W, 3).float(),
                                                      gt.to(device=device, dtype=torch.float32), "hip")
                psnr, ssim = float(np.mean(psnrs)), float(np.mean(ssims))
            print("PSNR: %.2f, SSIM: %.4f" % (psnr, ssim), flush=True)
            finish.write("%s %.2f %.4f 1\n" % (name, psnr, ssim))
        except Exception as e:   # eval.py:146-149: report the object and go on
            print("ERROR processing %s: %s" % (name, e), flush=True)
            traceback.print_exc()
    finish.close()


if __name__ == "__main__":
    main()
