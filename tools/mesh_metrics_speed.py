#!/usr/bin/env python
"""Times the scoring of an extracted mesh against a ground-truth mesh on one MI355X, three ways, at
the size the evaluation uses: 100,000 surface samples of each of two meshes extracted
(pnr.ops.marching_cubes) from synthetic 256^3 grids, the meshes resident on the device as
scripts/eval.py leaves them.

  device  pnr.ops.mesh_sample x 2, pnr.ops.nearest x 2, pnr.ops.mesh_distance_sums
          (csrc/meshdist.hip), each stage between HIP events; and the whole of
          pnr.evaluate.mesh_metrics(backend="hip") on the host clock (it ends in a read-back)
  host    what exists without the kernels: both meshes copied to the host, then
          pnr.evaluate.mesh_metrics(backend="numpy") (numpy sampling, scipy cKDTree)   (host clock)
  cdist   on the same device and the same sample points: torch.cdist in row chunks of --cdist_rows
          with a min per chunk, both directions (the n x m matrix is 40 GB and cannot exist whole)
          (HIP events)
Medians over --reps runs after --warmup; the device and cdist searches alternate inside one loop.
The shader clock is read (not set) before and after from the driver's sysfs table.

The file also records, for a near-pair case (4,096 queries 1e-3 away from rows of a 100,000-point
cloud in [-1, 1]^3), each route's maximum relative error of the nearest distance against an fp64
difference-form brute force.

  python tools/mesh_metrics_speed.py [--out profiles/meshdist/meshdist_speed.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "pixel-nerf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pnr import evaluate, ops  # noqa: E402
from speed_common import _stats, blob_grid, events, shader_clock_mhz  # noqa: E402


def cdist_nearest(a, b, rows):
    d, idx = [], []
    for i in range(0, a.shape[0], rows):
        m = torch.cdist(a[i:i + rows], b).min(1)
        d.append(m.values)
        idx.append(m.indices)
    return torch.cat(d), torch.cat(idx)


def near_pair_errors(dev, rows):
    rng = np.random.default_rng(1)
    b = rng.uniform(-1, 1, (100000, 3)).astype(np.float32)
    a = (b[:4096] + 1e-3 * rng.uniform(-1, 1, (4096, 3))).astype(np.float32)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    ref = torch.cat([((ta[i:i + 256, None, :].double() - tb[None, :, :].double()) ** 2).sum(-1).min(1).values
                     for i in range(0, 4096, 256)]).sqrt()
    d_dev = ops.nearest(ta, tb)[0].double().sqrt()
    d_cd = cdist_nearest(ta, tb, rows)[0].double()
    d_host = torch.from_numpy(np.sqrt(evaluate.nearest_np(a, b)[0])).to(dev)
    rel = lambda d: float(((d - ref).abs() / ref).max())   # noqa: E731
    return dict(queries=4096, cloud=100000, offset=1e-3, reference="fp64 differences, brute force, on the device",
                max_rel_err_distance=dict(device=rel(d_dev), cdist=rel(d_cd), host=rel(d_host)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--n_samples", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host_reps", type=int, default=20)
    ap.add_argument("--cdist_rows", type=int, default=4096, help="rows of a per torch.cdist call (1.6 GB at 100k)")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_metrics_speed.py needs a HIP device: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    n, tau = args.n_samples, 0.01
    clock_before = shader_clock_mhz()
    pred = ops.marching_cubes(blob_grid(args.res, dev, 0.05), 0.0, spacing=(2.0 / (args.res - 1),) * 3, origin=(-1.0,) * 3)
    gt = ops.marching_cubes(blob_grid(args.res, dev, 0.04), 0.0, spacing=(2.0 / (args.res - 1),) * 3, origin=(-1.0,) * 3)
    print("meshes: %d and %d faces" % (pred[1].shape[0], gt[1].shape[0]))

    # ---- device route, stage by stage ----
    def sampling():
        return ops.mesh_sample(pred[0], pred[1], n, 0), ops.mesh_sample(gt[0], gt[1], n, 1)

    (pa, na, _, _), (pb, nb, _, _) = sampling()

    def search():
        return ops.nearest(pa, pb), ops.nearest(pb, pa)

    (d2_ab, i_ab), (d2_ba, i_ba) = search()
    stage = dict(sampling_ms=_stats(events(sampling, args.warmup, args.reps)),
                 reduce_ms=_stats(events(lambda: ops.mesh_distance_sums(d2_ab, i_ab, d2_ba, i_ba, na, nb, tau),
                                         args.warmup, args.reps)))
    # the two searches alternate, so a drifting clock hits both alike
    s_ms, c_ms = [], []
    for i in range(args.warmup + args.reps):
        s = events(search, 0, 1)
        c = events(lambda: (cdist_nearest(pa, pb, args.cdist_rows), cdist_nearest(pb, pa, args.cdist_rows)), 0, 1)
        if i >= args.warmup:
            s_ms += s
            c_ms += c
    stage["search_ms"] = _stats(s_ms)
    cd = cdist_nearest(pa, pb, args.cdist_rows)
    same = float((cd[1] == i_ab).double().mean())

    def wall(fn, warmup, reps):
        ms, res = [], None
        for i in range(warmup + reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize(dev)
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms, res

    hip_ms, hip_scores = wall(lambda: evaluate.mesh_metrics(pred, gt, n, tau, 0, "hip"), args.warmup, args.reps)
    host_ms, host_scores = wall(lambda: evaluate.mesh_metrics(tuple(t.cpu().numpy() for t in pred),
                                                              tuple(t.cpu().numpy() for t in gt), n, tau, 0, "numpy"),
                                1, args.host_reps)
    spread = (stage["search_ms"]["max"] - stage["search_ms"]["min"]) + (max(c_ms) - min(c_ms))
    out = dict(device=torch.cuda.get_device_name(0), shader_clock_mhz=dict(before=clock_before, after=shader_clock_mhz()),
               grid=args.res, n_samples=n, tau=tau, faces=dict(pred=int(pred[1].shape[0]), gt=int(gt[1].shape[0])),
               warmup=args.warmup, reps=args.reps, host_threads=torch.get_num_threads(),
               device_route=dict(stages=stage, whole_call_wall_ms=_stats(hip_ms),
                                 tiles=dict(queries=ops.NEAREST_QUERIES, tile=ops.NEAREST_TILE, slice=ops.NEAREST_SLICE)),
               host_route=dict(whole_call_wall_ms=_stats(host_ms), search="scipy cKDTree"),
               cdist_route=dict(search_ms=_stats(c_ms), rows_per_call=args.cdist_rows,
                                share_of_indices_equal_to_device=same),
               search_device_over_cdist=stage["search_ms"]["median"] / statistics.median(c_ms),
               search_margin_ms=statistics.median(c_ms) - stage["search_ms"]["median"],
               search_spread_ms=spread, scores=dict(hip=hip_scores, numpy=host_scores),
               near_pairs=near_pair_errors(dev, args.cdist_rows))
    print(json.dumps(out, indent=1, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
