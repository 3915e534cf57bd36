#!/usr/bin/env python
"""Times the scoring step of an evaluation run on one MI355X, on the device (csrc/metrics.hip) and
on the host, at the three image stacks the evaluation scripts produce: the NMR batch
(24 x 64 x 64 x 3), an SRN frame (1 x 128 x 128 x 3) and a DTU frame (1 x 300 x 400 x 3).

Both routes start where a caller stands after a render: the rendered stack on the device, the
ground truth on the host.  Both end with Python floats on the host.
  numpy  ``.cpu().numpy()`` of the render (a stream sync and a device-to-host copy), then
         pnr.evaluate.psnr_np / ssim image by image            (host clock)
  hip    the ground truth to the device, pnr.ops.image_metrics, one (2, N) float64 readback
         = pnr.evaluate.image_metrics(..., "hip")              (host clock, ends in the readback)
  op     pnr.ops.image_metrics alone, inputs resident: allocation of the workspace and the
         outputs, two launches, the PSNR expression            (HIP events over --inner calls)
The two host-clock routes alternate inside one loop, after --warmup rounds; medians over --reps.
They are timed twice: for all shapes before any ``op`` loop has run in the process ("routes"),
and again after the ``op`` loops of all shapes ("routes_after_op_loops", 3 x (warmup + reps) x
inner back-to-back asynchronous calls later), because the second reading came out differently.

  python tools/metrics_speed.py [--out profiles/metrics/metrics_speed.json]
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

SHAPES = (("nmr_batch", (24, 64, 64, 3)), ("srn_frame", (1, 128, 128, 3)), ("dtu_frame", (1, 300, 400, 3)))


def _stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


class Case:
    def __init__(self, name, shape, dev):
        rng = np.random.default_rng(0)
        self.name, self.shape, self.dev = name, shape, dev
        self.gt = rng.random(shape, dtype=np.float32)
        pred = np.clip(self.gt + 0.1 * rng.standard_normal(shape, dtype=np.float32), 0.0, 1.0)
        self.pred = torch.from_numpy(pred).to(dev)
        self.gt_t = torch.from_numpy(self.gt)
        self.gt_dev = self.gt_t.to(dev)

    def routes(self, warmup, reps):
        """The two host-clock routes, alternating."""
        fns = (("numpy", lambda: evaluate.image_metrics(self.pred.cpu().numpy(), self.gt, "numpy")),
               ("hip", lambda: evaluate.image_metrics(self.pred, self.gt_t, "hip")))
        wall, res = dict(numpy=[], hip=[]), {}
        for i in range(warmup + reps):
            for key, fn in fns:
                torch.cuda.synchronize(self.dev)
                t0 = time.perf_counter()
                res[key] = fn()
                dt = (time.perf_counter() - t0) * 1e3
                if i >= warmup:
                    wall[key].append(dt)
        diff = [max(abs(a - b) for a, b in zip(res["hip"][k], res["numpy"][k])) for k in (0, 1)]
        out = dict(numpy_route_ms=_stats(wall["numpy"]), hip_route_ms=_stats(wall["hip"]),
                   hip_route_over_numpy_route=statistics.median(wall["hip"]) / statistics.median(wall["numpy"]),
                   max_abs_diff=dict(psnr_db=diff[0], ssim=diff[1]))
        print("%-10s %-12s numpy %7.3f ms  hip %7.3f ms (%.3fx)  |d psnr| %.1e |d ssim| %.1e" % (
            self.name, "x".join(map(str, self.shape)), out["numpy_route_ms"]["median"],
            out["hip_route_ms"]["median"], out["hip_route_over_numpy_route"], diff[0], diff[1]))
        return out

    def op(self, warmup, reps, inner):
        ms = []
        for i in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                ops.image_metrics(self.pred, self.gt_dev)
            b.record()
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b) / inner)
        print("%-10s %-12s op alone %.4f ms/call" % (self.name, "x".join(map(str, self.shape)), statistics.median(ms)))
        return _stats(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200, help="calls of the op between one pair of events")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("metrics_speed.py needs a HIP device: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    cases = [Case(n, s, dev) for n, s in SHAPES]
    runs = [dict(name=c.name, shape=list(c.shape)) for c in cases]
    print("routes, before any op loop")
    for c, r in zip(cases, runs):
        r["routes"] = c.routes(args.warmup, args.reps)
    for c, r in zip(cases, runs):
        r["op_ms_per_call"] = c.op(args.warmup, args.reps, args.inner)
    print("routes again, after the op loops")
    for c, r in zip(cases, runs):
        r["routes_after_op_loops"] = c.routes(args.warmup, args.reps)
    out = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps,
               op_calls_per_event_pair=args.inner, host_threads=torch.get_num_threads(), runs=runs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
