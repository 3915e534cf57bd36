#!/usr/bin/env python
"""Speed and image difference of mlp_precision = "f16" against "f16x3" on one MI355X.

The batch is bench.py's cfg3 step: one 64 x 64 NMR source view encoded, 24 target frames =
98,304 rays x (64 coarse + 64 fine) rendered in 50,000-ray chunks, the encode included.  One
process, one net; after a warm-up of both modes the two are timed alternately, WINDOWS times each,
in windows of at least WINDOW_S seconds closed by a synchronise.  Reported:

  * rays/s of every window, the ratio of the medians and the spread within each mode
    ((max - min) / median);
  * the fine launch's mean HIP-event time per mode and its share of the mode's MFMA peak
    (2.5 PFLOP/s for one fp16 product per FMA, 833 TFLOP/s fp32-equivalent for f16x3's three);
  * PSNR and max |d| of the f16 fine rgb against the f16x3 fine rgb of the same seeded call, and
    the same PSNR after both are rounded to 8 bits.

    python tools/precision_speed.py [--out profiles/<tag>/precision_speed.json]

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "pixel-nerf_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402
from pnr.renderer import NeRFRenderer  # noqa: E402

MODES = ("f16x3", "f16")
# fp32-equivalent MFMA peak of each mode: the dense fp16 / bf16 rate over its products per FMA
PEAK_TFLOPS = {"f16x3": bench.MFMA_BF16_PEAK_TFLOPS / 3, "f16": bench.MFMA_BF16_PEAK_TFLOPS}


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else 10.0 * math.log10(1.0 / mse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5, help="timed windows per mode (>= 5)")
    ap.add_argument("--window-s", type=float, default=1.0, help="minimum seconds per window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.windows >= 5 and args.window_s >= 1.0, "at least 5 windows of at least 1 s per mode"

    dev = torch.device("cuda:0")
    probe = bench.RenderProbe(bench.HipEvents())
    net = bench.make_net(dev, "f16x3", True, use_first_pool=False)
    net.encoder.infer_fast = True
    img, src, focal, rays = bench.nmr_inputs(dev)
    n_rays = rays.shape[0]
    renderer = NeRFRenderer(n_coarse=bench.KC, n_fine=bench.KF, white_bkgd=True,
                            eval_batch_size=bench.RAY_BATCH).to(dev)
    render_par = renderer.bind_parallel(net, simple_output=True).eval()
    torch.backends.cudnn.benchmark = True

    def step():
        net.encode(img, src, focal)
        return torch.cat([render_par(r[None])[0][0] for r in torch.split(rays, bench.RAY_BATCH, dim=0)])

    def window(mode):
        net.mlp_precision = mode
        torch.cuda.synchronize(dev)
        probe.reset()
        probe.on = True
        n, t0 = 0, time.perf_counter()
        while True:
            step()
            n += 1
            if time.perf_counter() - t0 >= args.window_s:   # host time runs ahead of the queue:
                torch.cuda.synchronize(dev)                  # close the window on the device's
                if time.perf_counter() - t0 >= args.window_s:
                    break
        dt = time.perf_counter() - t0
        probe.on = False
        avg, _ = probe.summary("f16x3", True)   # per-kernel event means of this window's launches
        pts = sum(c[1] * (c[2] + c[3]) for c in probe.calls) / len(probe.calls)
        return n * n_rays / dt, avg["mlp_fine"], avg["mlp_coarse"], pts

    res = {"workload": "cfg3: 24 NMR 64 x 64 frames = %d rays x (64 + 64), encode included, %d-ray chunks"
                       % (n_rays, bench.RAY_BATCH),
           "windows_per_mode": args.windows, "window_s_min": args.window_s, "modes": {}}
    with torch.no_grad():
        rgb = {}
        for mode in MODES:                       # warm-up of both modes + the seeded comparison call
            net.mlp_precision = mode
            step()
            torch.manual_seed(1234)
            rgb[mode] = step().float().cpu()
        torch.cuda.synchronize(dev)
        rows = {m: [] for m in MODES}
        for _ in range(args.windows):            # alternate: a drifting clock hits both modes alike
            for mode in MODES:
                rows[mode].append(window(mode))
    flop_pt = bench.flop_per_point(1, True)
    for mode in MODES:
        rps = [r[0] for r in rows[mode]]
        s = sorted(rps)
        med = s[len(s) // 2]
        fine_ms = sum(r[1] for r in rows[mode]) / len(rows[mode])
        coarse_ms = sum(r[2] for r in rows[mode]) / len(rows[mode])
        pts = rows[mode][0][3]
        tflops = pts * flop_pt / (fine_ms * 1e-3) / 1e12
        res["modes"][mode] = {
            "rays_per_s": [round(v, 1) for v in rps], "median": round(med, 1),
            "spread": round((s[-1] - s[0]) / med, 4),
            "fine_launch_ms": round(fine_ms, 4), "coarse_launch_ms": round(coarse_ms, 4),
            "fine_points_per_launch": round(pts, 1),
            "fine_tflops_fp32_equivalent": round(tflops, 1), "peak_tflops": round(PEAK_TFLOPS[mode], 1),
            "fine_frac_of_peak": round(tflops / PEAK_TFLOPS[mode], 4)}
    a, b = res["modes"]["f16x3"], res["modes"]["f16"]
    res["speedup_median"] = round(b["median"] / a["median"], 4)
    res["fine_launch_speedup"] = round(a["fine_launch_ms"] / b["fine_launch_ms"], 4)
    res["max_spread"] = max(a["spread"], b["spread"])
    res["faster_by_more_than_spread"] = bool(res["speedup_median"] - 1.0 > res["max_spread"])
    q = lambda t: torch.round(t.clamp(0, 1) * 255.0) / 255.0   # noqa: E731
    d = (rgb["f16"] - rgb["f16x3"]).abs()
    res["image"] = {"what": "f16 fine rgb against f16x3 fine rgb of the same seeded call (%d rays)" % n_rays,
                    "psnr_db": round(psnr(rgb["f16"], rgb["f16x3"]), 2), "max_abs": float(d.max()),
                    "mean_abs": float(d.mean()),
                    "psnr_8bit_db": round(psnr(q(rgb["f16"]), q(rgb["f16x3"])), 2),
                    "pixels_differing_8bit": int((q(rgb["f16"]) != q(rgb["f16x3"])).any(-1).sum())}
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))
    return 0 if res["faster_by_more_than_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
