#!/usr/bin/env python
"""Times the containment test behind the volumetric IoU on one MI355X, three ways, at the size the
evaluation uses: 100,000 uniform points (pnr.ops.box_sample) in the padded bounds of two meshes
extracted (pnr.ops.marching_cubes) from the synthetic 256^3 grids of tools/mesh_metrics_speed.py,
resident on the device as scripts/eval.py leaves them, each point scored against each mesh.

  kernel  pnr.ops.winding_number x 2 (csrc/winding.hip)                                (HIP events)
  torch   the same formula as chunked torch ops on the same device, fp32 pairs and an fp64 sum,
          --torch_rows queries at a time (a dozen rows x faces temporaries per step)   (HIP events)
  host    pnr.evaluate.winding_np (numpy, fp64) on --host_points of the points, timed on the host
          clock and scaled to all of them (the JSON says so)
Medians over --reps runs after --warmup; the kernel and the torch route alternate inside one loop.
The shader clock is read (not set) before and after from the driver's sysfs table.

The file also records the pairs per second the kernel reaches beside the VALU issue bound of its
inner loop (--valu_per_pair vector instructions per pair, read from the build's device assembly; one
wave64 instruction issues in two cycles per SIMD with two or more waves resident), the largest
difference between the routes' winding numbers, and pnr.evaluate.volume_iou(backend="hip") on the
host clock.

  python tools/winding_speed.py [--out profiles/winding/winding_speed.json]
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

from pnr import evaluate, ops  # noqa: E402
from speed_common import _stats, blob_grid, events, shader_clock_mhz  # noqa: E402

SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 256 * 4, 2.4e9, 2   # MI355X: 256 CUs x 4 SIMDs, 2.4 GHz peak


def torch_winding(verts, faces, points, rows):
    """pnr_winding's pair formula in torch: fp32 pairs, the angles summed in fp64."""
    tri = verts[faces.long()]                                  # (T, 3, 3)
    A, B, C = tri[:, 0][None], tri[:, 1][None], tri[:, 2][None]
    out = []
    for i in range(0, points.shape[0], rows):
        q = points[i:i + rows, None, :]
        a, b, c = A - q, B - q, C - q
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = (a * torch.linalg.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out.append((2.0 * torch.atan2(num, den)).sum(-1, dtype=torch.float64))
    return torch.cat(out) / (4.0 * np.pi)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--n_points", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch_rows", type=int, default=256, help="queries per step of the torch route")
    ap.add_argument("--host_points", type=int, default=200, help="points the host route scores (scaled up)")
    ap.add_argument("--valu_per_pair", type=float, default=131.0,
                    help="vector instructions per pair in k_winding's inner loop (build/winding.hip.gfx950.s)")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("winding_speed.py needs a HIP device: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    n = args.n_points
    clock_before = shader_clock_mhz()
    sp, org = (2.0 / (args.res - 1),) * 3, (-1.0,) * 3
    pred = ops.marching_cubes(blob_grid(args.res, dev, 0.05), 0.0, spacing=sp, origin=org)
    gt = ops.marching_cubes(blob_grid(args.res, dev, 0.04), 0.0, spacing=sp, origin=org)
    both = torch.cat([pred[0], gt[0]])
    lo, hi = evaluate._grown_box(both.min(0).values.cpu().numpy(), both.max(0).values.cpu().numpy(), 0.05)
    pts = ops.box_sample(lo.tolist(), hi.tolist(), n, 0, device=dev)
    faces = int(pred[1].shape[0]) + int(gt[1].shape[0])
    pairs = float(n) * faces
    print("meshes: %d and %d faces, %d points, %.3g pairs" % (pred[1].shape[0], gt[1].shape[0], n, pairs))

    def kernel():
        return ops.winding_number(pred[0], pred[1], pts), ops.winding_number(gt[0], gt[1], pts)

    def chunked():
        return torch_winding(pred[0], pred[1], pts, args.torch_rows), torch_winding(gt[0], gt[1], pts, args.torch_rows)

    w_k, w_t = kernel(), chunked()
    k_ms, t_ms = [], []
    for i in range(args.warmup + args.reps):   # alternating, so a drifting clock hits both alike
        k = events(kernel, 0, 1)
        t = events(chunked, 0, 1)
        if i >= args.warmup:
            k_ms += k
            t_ms += t
    sub = pts[:args.host_points].cpu().numpy()
    host_mesh = [tuple(t.cpu().numpy() for t in m) for m in (pred, gt)]
    t0 = time.perf_counter()
    w_h = [evaluate.winding_np(v, f, sub) for v, f in host_mesh]
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    iou = evaluate.volume_iou(pred, gt, n_points=n, seed=0, backend="hip")
    torch.cuda.synchronize(dev)
    iou_s = time.perf_counter() - t0

    k_med, t_med = statistics.median(k_ms), statistics.median(t_ms)
    bound_pairs_s = SIMDS * 64.0 / (args.valu_per_pair * CYCLES_PER_VALU) * CLOCK_HZ
    diff = lambda a, b: float(max((x - y).abs().max() for x, y in zip(a, b)))   # noqa: E731
    w_h_dev = [torch.from_numpy(w).to(dev) for w in w_h]
    out = dict(device=torch.cuda.get_device_name(0), shader_clock_mhz=dict(before=clock_before, after=shader_clock_mhz()),
               grid=args.res, n_points=n, faces=dict(pred=int(pred[1].shape[0]), gt=int(gt[1].shape[0])), pairs=pairs,
               warmup=args.warmup, reps=args.reps, host_threads=torch.get_num_threads(),
               kernel_route=dict(ms=_stats(k_ms), pairs_per_s=pairs / (k_med * 1e-3),
                                 tiles=dict(queries=ops.WINDING_QUERIES, tile=ops.WINDING_TILE, slice=ops.WINDING_SLICE)),
               torch_route=dict(ms=_stats(t_ms), rows_per_step=args.torch_rows, pairs_per_s=pairs / (t_med * 1e-3)),
               host_route=dict(points_scored=int(len(sub)), seconds_scored=host_s,
                               ms_scaled_to_all_points=host_s * 1e3 * n / len(sub),
                               note="winding_np on a subsample, its time scaled by n_points / points_scored"),
               kernel_over_torch=k_med / t_med, margin_ms=t_med - k_med,
               spread_ms=(max(k_ms) - min(k_ms)) + (max(t_ms) - min(t_ms)),
               valu_issue_bound=dict(valu_per_pair=args.valu_per_pair, cycles_per_wave64_valu=CYCLES_PER_VALU, simds=SIMDS,
                                     clock_hz=CLOCK_HZ, pairs_per_s=bound_pairs_s, ms=pairs / bound_pairs_s * 1e3,
                                     kernel_share_of_bound=pairs / (k_med * 1e-3) / bound_pairs_s,
                                     note="every vector instruction counted as one two-cycle issue at the peak clock; "
                                          "transcendentals (3 v_sqrt, 1 v_rcp per pair) and the fp64 add cost more"),
               max_abs_difference=dict(kernel_vs_torch=diff(w_k, w_t),
                                       kernel_vs_host_fp64=diff([w[:len(sub)] for w in w_k], w_h_dev)),
               volume_iou_hip=dict(scores=iou, wall_ms_first_call=iou_s * 1e3))
    print(json.dumps(out, indent=1, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
