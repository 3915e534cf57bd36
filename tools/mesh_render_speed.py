#!/usr/bin/env python
"""Times the mesh rendering on one MI355X, three ways, on three workloads:

  mesh128  the cleaned 256^3-grid mesh of tools/mesh_clean_speed.py (two blobs, floaters removed with
           pnr.evaluate.clean_mesh), normalised to the radius scripts/render_meshes.py uses, from the 128
           cameras of pnr.evaluate.sphere_poses at 128 x 128 (f = 131.25)
  mesh512  the same mesh and cameras at 512 x 512 (f = 525)
  box512   a 12-face box at 512 x 512: every face takes the wave path

  kernel  pnr.ops.mesh_raster, and pnr.ops.mesh_shade on its output (csrc/meshraster.hip)   (HIP events)
  torch   the same hit rule as chunked torch ops on the same device, brute force over all faces,
          --torch_rows pixels at a time, on --torch_views of the views (the JSON states the count; the
          time is NOT scaled to all views)                                                  (HIP events)
  host    pnr.evaluate.raycast_np (numpy, fp64) on ONE view at --host_size x --host_size pixels, on the
          host clock (the JSON states the rays and pairs; nothing is scaled)
Medians over --reps runs after --warmup; the routes alternate inside one loop.  The shader clock is read
(not set) before and after.  The file also records an A/B of the threshold between the lane path and the
wave path (pnr_mesh_raster_set_small; the values alternate inside one loop on the same box), the least
bytes each pass moves, and that the kernel and the torch route agree.

  python tools/mesh_render_speed.py [--out profiles/meshraster/meshraster_speed.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "pixel-nerf_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pnr import evaluate, mesh, ops  # noqa: E402
from speed_common import _stats, events, floater_grid, shader_clock_mhz  # noqa: E402

LIGHTS = dict(lights=[(1.3, 1.3, 1.3), (-1.3, -1.3, 1.3), (0.0, -1.3, 1.3)], weights=[0.55, 0.18, 0.11], ambient=0.15)


def torch_raster(verts, faces, poses, size, focal, rows):
    """pnr_mesh_raster's hit rule in torch, brute force, in the dtype of `verts` (fp32: the route that is
    timed; fp64: the check of both): (hit (NV, H, W) bool, depth (NV, H, W))."""
    c = 0.5 * size
    poses = poses.to(verts.dtype)
    j, i = torch.meshgrid(torch.arange(size, device=verts.device, dtype=verts.dtype),
                          torch.arange(size, device=verts.device, dtype=verts.dtype), indexing="ij")
    X, Yn = ((i - c) / focal).reshape(-1, 1), (-((j - c) / focal)).reshape(-1, 1)
    length = torch.sqrt(X * X + Yn * Yn + 1.0).reshape(-1)
    tri = verts[faces.long()]
    hits, depths = [], []
    for p in poses:
        cam = (tri - p[:3, 3]) @ p[:3, :3]
        a, b, cc = cam[:, 0], cam[:, 1], cam[:, 2]
        n_ab, n_bc, n_ca = torch.linalg.cross(a, b), torch.linalg.cross(b, cc), torch.linalg.cross(cc, a)
        best = []
        for r in range(0, X.shape[0], rows):
            x, y = X[r:r + rows], Yn[r:r + rows]
            e_ab = x * n_ab[:, 0] + y * n_ab[:, 1] - n_ab[:, 2]
            e_bc = x * n_bc[:, 0] + y * n_bc[:, 1] - n_bc[:, 2]
            e_ca = x * n_ca[:, 0] + y * n_ca[:, 1] - n_ca[:, 2]
            lo = torch.minimum(torch.minimum(e_ab, e_bc), e_ca)
            hi = torch.maximum(torch.maximum(e_ab, e_bc), e_ca)
            det = e_ab + e_bc + e_ca
            s = -(e_bc * a[:, 2] + e_ca * b[:, 2] + e_ab * cc[:, 2]) / det
            ok = ~((lo < 0) & (hi > 0)) & (det != 0) & (s > 0) & torch.isfinite(s)
            best.append(torch.where(ok, s, torch.full_like(s, float("inf"))).min(1).values)
        s = torch.cat(best)
        hits.append(torch.isfinite(s).reshape(size, size))
        depths.append(torch.where(torch.isfinite(s), s * length, torch.zeros_like(s)).reshape(size, size))
    return torch.stack(hits), torch.stack(depths)


def kernel_times(names, reps):
    """Median device time per kernel (microseconds) from torch's profiler, or None where it sees none."""
    def run(fn):
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            out = {}
            for ev in prof.events():
                for n in names:
                    if n in ev.name and getattr(ev, "device_time", getattr(ev, "cuda_time", 0)) > 0:
                        out.setdefault(n, []).append(float(getattr(ev, "device_time", getattr(ev, "cuda_time", 0))))
            return {n: dict(median_us=statistics.median(v), launches=len(v)) for n, v in out.items()} or None
        except Exception as e:   # noqa: BLE001 -- a profiler that does not load is recorded, not fatal
            return dict(error=repr(e)[:200])
    return run


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--floaters", type=int, default=300)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch_views", type=int, default=2, help="views the torch route renders (not scaled up)")
    ap.add_argument("--torch_rows", type=int, default=256, help="pixels per step of the torch route")
    ap.add_argument("--host_size", type=int, default=16, help="image side of the host route's one view")
    ap.add_argument("--small", type=int, nargs="*", default=[0, 1, 4, 8, 16, 32, 64, 256, 1 << 30],
                    help="thresholds of the lane path / wave path A/B")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render_speed.py needs a HIP device: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    clock_before = shader_clock_mhz()
    verts, faces = ops.marching_cubes(floater_grid(args.res, dev, args.floaters), 0.0)
    soup = verts[faces.long()].reshape(-1, 3).contiguous()
    soup_faces = torch.arange(soup.shape[0], device=dev, dtype=torch.int32).reshape(-1, 3)
    cv, cf, info = evaluate.clean_mesh(soup, soup_faces, keep="largest", backend="hip")
    radius = 0.95 * 1.3 * float(np.sin(np.arctan(64.0 / 131.25)))
    cv = mesh.normalize_bounds(cv, radius).contiguous()
    bv = torch.tensor([[x, y, z] for x in (-.35, .35) for y in (-.35, .35) for z in (-.35, .35)], device=dev)
    bf = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                       [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], device=dev, dtype=torch.int32)
    poses = torch.from_numpy(evaluate.sphere_poses(args.views, 1.3)[0]).float().to(dev)
    n_t, n_v = int(cf.shape[0]), int(cv.shape[0])
    print("mesh: %d faces, %d vertices (%s)" % (n_t, n_v, info))
    loads = {"mesh128": (cv, cf, 128, 131.25), "mesh512": (cv, cf, 512, 525.0), "box512": (bv, bf, 512, 525.0)}
    prof = kernel_times(("k_raster_fill", "k_raster_cover", "k_raster_resolve", "k_raster_shade"), 3)
    out_loads = {}
    for name, (v, f, size, focal) in loads.items():
        t_f = int(f.shape[0])
        face, depth = ops.mesh_raster(v, f, poses, size, size, focal)

        def raster():
            return ops.mesh_raster(v, f, poses, size, size, focal)

        def shade():
            return ops.mesh_shade(v, f, poses, size, size, focal, face, depth, **LIGHTS)

        tv = poses[:args.torch_views]

        def chunked():
            return torch_raster(v, f, tv, size, focal, args.torch_rows)

        ms = {"raster": [], "shade": [], "torch": []}
        with_torch = name != "mesh512"            # the 512 x 512 brute force adds minutes and no information
        for i in range(args.warmup + args.reps):   # alternating, so a drifting clock hits all alike
            for k, fn in (("raster", raster), ("shade", shade)) + ((("torch", chunked),) if with_torch else ()):
                t = events(fn, 0, 1)
                if i >= args.warmup:
                    ms[k] += t
        ab = {s: [] for s in args.small}
        for i in range(args.warmup + args.reps):
            for s in args.small:
                with ops.raster_small_pixels(s):
                    t = events(raster, 0, 1)
                if i >= args.warmup:
                    ab[s] += t
        covered = int((face >= 0).sum())
        n_pix = int(face.numel())
        entry = dict(faces=t_f, views=args.views, size=size, focal=focal, pixels=n_pix, covered_share=covered / n_pix,
                     kernel_route=dict(raster_ms=_stats(ms["raster"]), shade_ms=_stats(ms["shade"]),
                                       per_kernel=prof(lambda: (raster(), shade())),
                                       face_view_pairs_per_s=t_f * args.views / (statistics.median(ms["raster"]) * 1e-3)),
                     min_bytes_per_pass=dict(
                         fill=8 * n_pix, resolve=8 * n_pix + 8 * n_pix,
                         cover_reads=(12 + 36) * t_f * args.views,
                         cover_atomics_at_least=covered,
                         shade=8 * n_pix + 12 * n_pix + 48 * covered,
                         note="cover: the face's indices and its three gathered vertices once per (view, face), then "
                              "one 8-byte pre-read per hit pair and one 8-byte atomic min where the key improves, at "
                              "least one per covered pixel; the gathers are served by the L2"),
                     small_threshold_ab={str(s): _stats(v) for s, v in ab.items()})
        if with_torch:
            hit_t, depth_t = chunked()
            same = bool(torch.equal(hit_t, face[:args.torch_views] >= 0))
            diff = float((depth_t - depth[:args.torch_views]).abs().max())
            # which of the two is right where they differ: the same brute force in fp64 on the same views
            hit_d, depth_d = torch_raster(v.double(), f, tv, size, focal, args.torch_rows)

            def against_fp64(hit, dep):
                both = hit & hit_d
                rel = ((dep.double() - depth_d).abs() / depth_d.clamp(min=1e-30))[both]
                return dict(pixels=int(hit_d.numel()), hit_miss_differs=int((hit != hit_d).sum()),
                            depth_off_by_more_than_1e_4=int((rel > 1e-4).sum()),
                            max_rel_depth_difference_elsewhere=float(rel[rel <= 1e-4].max()) if both.any() else 0.0)

            entry["against_fp64_brute_force"] = dict(views=args.torch_views,
                                                     kernel=against_fp64(face[:args.torch_views] >= 0,
                                                                         depth[:args.torch_views]),
                                                     torch_fp32=against_fp64(hit_t, depth_t))
            entry["torch_route"] = dict(ms=_stats(ms["torch"]), views_rendered=args.torch_views, rows_per_step=args.torch_rows,
                                        note="brute force over all faces on views_rendered views only; not scaled",
                                        ms_per_view=statistics.median(ms["torch"]) / args.torch_views,
                                        kernel_ms_per_view=statistics.median(ms["raster"]) / args.views,
                                        same_silhouette_as_kernel=same, max_abs_depth_difference=diff)
        out_loads[name] = entry
        print(name, json.dumps({k: entry[k] for k in ("kernel_route", "small_threshold_ab")}, sort_keys=True))
    # the host route: one view, a small image, all faces of the mesh
    hv, hf = cv.cpu().numpy(), cf.cpu().numpy()
    hs = args.host_size
    t0 = time.perf_counter()
    face_h, depth_h = evaluate.raycast_np(hv, hf, poses[:1].cpu().numpy(), hs, hs, 131.25 * hs / 128.0)
    host_s = time.perf_counter() - t0
    face_k, depth_k = ops.mesh_raster(cv, cf, poses[:1], hs, hs, 131.25 * hs / 128.0)
    host = dict(views=1, size=hs, rays=hs * hs, pairs=hs * hs * n_t, seconds=host_s, pairs_per_s=hs * hs * n_t / host_s,
                same_silhouette_as_kernel=bool(np.array_equal(face_h >= 0, face_k.cpu().numpy() >= 0)),
                max_abs_depth_difference=float(np.abs(depth_h - depth_k.cpu().numpy()).max()),
                note="raycast_np on one view of %d x %d pixels against all faces; nothing is scaled" % (hs, hs))
    out = dict(device=torch.cuda.get_device_name(0), shader_clock_mhz=dict(before=clock_before, after=shader_clock_mhz()),
               grid=args.res, floaters=args.floaters, warmup=args.warmup, reps=args.reps,
               host_threads=torch.get_num_threads(), mesh=dict(faces=n_t, vertices=n_v, radius=radius, clean=info),
               constants=dict(block=ops.RASTER_BLOCK, tile=ops.RASTER_TILE, small_pixels=ops.RASTER_SMALL_PIXELS),
               workloads=out_loads, host_route=host)
    print(json.dumps(out, indent=1, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
