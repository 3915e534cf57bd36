#!/usr/bin/env python
"""A folder of STL meshes to an SRN-layout dataset of rendered views: the step the reference does with
Blender (headless_Blender.py, Blender_cli.py, newBlender.py), here on the device with
pnr.ops.mesh_raster / mesh_shade (csrc/meshraster.hip), or on the host with --backend numpy.

  python scripts/render_meshes.py -M <dir of .stl> -D <out> [--prefix NAME] [--views 128] [--size 128] \
      [--focal 131.25] [--cam_radius 1.3] [--object_radius R] [--ssaa 2] [--backend auto|hip|numpy] \
      [--write_depth] [--overwrite]

For every ``<name>.stl`` of -M the mesh is centred by its bounds and scaled so that its farthest vertex
lies at --object_radius (pnr.mesh.normalize_bounds; the default radius is the largest whose sphere the
cameras see whole, times 0.95), and rendered from the --views cameras of pnr.evaluate.sphere_poses at
--cam_radius: the reference's golden spiral, 2 x views points, the upper half, each looking at the
origin.  View i goes to the split the reference sends it to: with (i + 1) % 10, 0 is test, 1 is val,
everything else train.  Under ``<out>/<prefix>_{train,val,test}/<name>/`` (prefix: the basename of
<out>, which is what pnr.data.SRNDataset(<out>) looks for):

  rgb/%06d.png     8-bit RGB on a white background; no fully covered pixel is white (colours stop at 254)
  pose/%06d.txt    camera-to-world in the file convention (OpenCV axes), 4 rows of %.16f
  intrinsics.txt   the reference's four lines: "fx cx cy 0.", "0. fy cy 0.", "0. 0. 1.", "H W"
  near_far.txt     "near far" = max(cam_radius - object_radius, 0.1), cam_radius + object_radius
  depth/%06d.npy   with --write_depth: float32 (H, W) distance along the pixel's ray at --ssaa 1, 0 = no hit

Lighting: the reference's three lights at cam_radius x {(1, 1, 1), (-1, -1, 1), (0, -1, 1)} as point
lights with weights in the ratio 1500 : 500 : 300 that sum to --light_gain, plus --ambient, on a flat
--albedo.  --ssaa k renders k x k samples per pixel, centred on the pixel's ray, and averages them.
An object whose train folder already holds intrinsics.txt is skipped unless --overwrite.
"""
import argparse
import math
import os
import os.path as osp
import shutil
import sys

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.join(REPO, "pixel-nerf_amd"))

import numpy as np  # noqa: E402

SPLITS = ("train", "val", "test")
LIGHT_DIRS = ((1.0, 1.0, 1.0), (-1.0, -1.0, 1.0), (0.0, -1.0, 1.0))
LIGHT_RATIO = (1500.0, 500.0, 300.0)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Render STL meshes into an SRN-layout dataset.")
    ap.add_argument("--mesh_dir", "-M", type=str, required=True, help="folder of <name>.stl")
    ap.add_argument("--datadir", "-D", type=str, required=True, help="dataset root to write")
    ap.add_argument("--prefix", type=str, default=None, help="split folder prefix (default: basename of -D)")
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--size", type=int, default=128, help="image side in pixels")
    ap.add_argument("--focal", type=float, default=131.25)
    ap.add_argument("--cam_radius", type=float, default=1.3)
    ap.add_argument("--object_radius", type=float, default=None,
                    help="radius the mesh is scaled to (default: 0.95 x the largest the cameras see whole)")
    ap.add_argument("--ssaa", type=int, default=2, help="k x k samples per pixel")
    ap.add_argument("--albedo", type=float, nargs=3, default=(0.8, 0.8, 0.8))
    ap.add_argument("--ambient", type=float, default=0.15)
    ap.add_argument("--light_gain", type=float, default=0.85, help="sum of the three light weights")
    ap.add_argument("--backend", choices=("auto", "hip", "numpy"), default="auto")
    ap.add_argument("--gpu_id", type=int, default=0, help="GPU id (hip backend)")
    ap.add_argument("--write_depth", action="store_true", help="also save depth/%%06d.npy")
    ap.add_argument("--overwrite", action="store_true")
    return ap.parse_args(argv)


def default_object_radius(cam_radius, size, focal):
    """0.95 x the radius of the largest origin-centred sphere inside every camera's field of view."""
    return 0.95 * cam_radius * math.sin(math.atan(0.5 * size / focal))


def split_of(i):
    """The reference's rule: with (i + 1) % 10, 0 is test, 1 is val, everything else train."""
    rem = (i + 1) % 10
    return "test" if rem == 0 else "val" if rem == 1 else "train"


def lights_of(cam_radius, gain):
    total = sum(LIGHT_RATIO)
    return ([tuple(cam_radius * x for x in d) for d in LIGHT_DIRS], [gain * r / total for r in LIGHT_RATIO])


def write_intrinsics(path, fx, fy, cx, cy, size):
    lines = ["%.6f %.6f %.6f 0." % (fx, cx, cy), "0. %.6f %.6f 0." % (fy, cy), "0. 0. 1.", "%d %d" % (size, size)]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def write_pose(path, c2w):
    with open(path, "w") as f:
        for row in np.asarray(c2w, np.float64).reshape(4, 4):
            f.write(" ".join("%.16f" % v for v in row) + "\n")


def render_object(verts, faces, poses, args, backend):
    """(rgb (NV, H, W, 3) uint8, depth (NV, H, W) float32 or None) of the normalised mesh."""
    import torch

    from pnr import evaluate

    lights, weights = lights_of(args.cam_radius, args.light_gain)
    c = 0.5 * args.size
    kw = dict(lights=lights, weights=weights, albedo=tuple(args.albedo), ambient=args.ambient,
              background=(1.0, 1.0, 1.0))
    p32 = torch.from_numpy(poses.astype(np.float32))
    out = evaluate.render_mesh_views(verts, faces, p32, args.size, args.size, args.focal, c=(c, c), ssaa=args.ssaa,
                                     backend=backend, **kw)
    rgb = torch.round(out["rgb"].clamp(0.0, 1.0) * 255.0).to(torch.uint8).cpu().numpy()
    depth = None
    if args.write_depth:
        if args.ssaa == 1:
            depth = out["depth"]
        else:
            depth = evaluate.render_mesh_views(verts, faces, p32, args.size, args.size, args.focal, c=(c, c), ssaa=1,
                                               backend=backend, **kw)["depth"]
        depth = depth.float().cpu().numpy()
    return rgb, depth


def main(argv=None):
    args = parse_args(argv)
    if args.views < 1 or args.size < 1 or args.ssaa < 1:
        raise SystemExit("render_meshes: --views, --size and --ssaa must be >= 1")
    if args.object_radius is None:
        args.object_radius = default_object_radius(args.cam_radius, args.size, args.focal)
    if not 0.0 < args.object_radius < args.cam_radius:
        raise SystemExit("render_meshes: --object_radius must lie in (0, --cam_radius)")
    from PIL import Image

    from pnr import evaluate, mesh

    backend = evaluate._resolve_backend(args.backend, "render")
    if backend == "hip":
        import torch

        torch.cuda.set_device(args.gpu_id)
    print("Rendering with the", backend, "backend")
    prefix = args.prefix or osp.basename(osp.normpath(args.datadir))
    poses, file_poses = evaluate.sphere_poses(args.views, args.cam_radius)
    names = sorted(x[:-4] for x in os.listdir(args.mesh_dir) if x.lower().endswith(".stl"))
    if not names:
        raise SystemExit("render_meshes: no .stl under %s" % args.mesh_dir)
    c = 0.5 * args.size
    near, far = max(args.cam_radius - args.object_radius, 0.1), args.cam_radius + args.object_radius
    done = 0
    for name in names:
        dirs = {s: osp.join(args.datadir, "%s_%s" % (prefix, s), name) for s in SPLITS}
        if osp.isfile(osp.join(dirs["train"], "intrinsics.txt")) and not args.overwrite:
            print("render_meshes: %s exists; skipped (use --overwrite)" % name)
            continue
        verts, faces = mesh.read_stl_indexed(osp.join(args.mesh_dir, name + ".stl"))
        if len(faces) == 0:
            print("render_meshes: %s has no triangles; skipped" % name, file=sys.stderr)
            continue
        verts = mesh.normalize_bounds(verts, args.object_radius)
        rgb, depth = render_object(verts, faces, poses, args, backend)
        for s in SPLITS:
            for sub in ("rgb", "pose") + (("depth",) if args.write_depth else ()):
                shutil.rmtree(osp.join(dirs[s], sub), ignore_errors=True)
                os.makedirs(osp.join(dirs[s], sub))
            write_intrinsics(osp.join(dirs[s], "intrinsics.txt"), args.focal, args.focal, c, c, args.size)
            with open(osp.join(dirs[s], "near_far.txt"), "w") as f:
                f.write("%.6f %.6f" % (near, far))
        counters = dict.fromkeys(SPLITS, 0)
        for i in range(args.views):
            s = split_of(i)
            idx = counters[s]
            counters[s] += 1
            write_pose(osp.join(dirs[s], "pose", "%06d.txt" % idx), file_poses[i])
            Image.fromarray(rgb[i], "RGB").save(osp.join(dirs[s], "rgb", "%06d.png" % idx))
            if depth is not None:
                np.save(osp.join(dirs[s], "depth", "%06d.npy" % idx), depth[i])
        print("%s: %d faces, %d views (%s)" % (name, len(faces), args.views,
                                                ", ".join("%s %d" % (s, counters[s]) for s in SPLITS)), flush=True)
        done += 1
    print(">>> RENDERED", done, "OBJECTS")


if __name__ == "__main__":
    main()
