#!/usr/bin/env python
"""Diagnostic (GPU): host time of the Python layer above the ABI, where the kernels are too small to hide it.

  python tools/host_time.py OUT.json

Two figures, each the median wall time per call of 200 calls after 20 warm-ups, the calls queued back to back
with one synchronisation at the end (so a call's time is what the host spends issuing it):
  render      NeRFRenderer.forward under no_grad, 256 rays x (8 + 8), counter RNG, one 32 x 32 source view
  train_step  forward under autograd, loss, backward and an Adam step, 128 rays x (8 + 8)
It uses names every revision of the layer has, so the file also runs from an older checkout against the same
library (PNR_LIB_PATH / PNR_TORCH_LIB_PATH); alternate the checkouts by process."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "pixel-nerf_amd"), REPO):
    sys.path.insert(0, p)

WARMUP, CALLS = 20, 200


def timed(step):
    import torch

    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    us = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        step()
        us.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    us.sort()
    return {"median_us": us[len(us) // 2], "min_us": us[0], "p90_us": us[int(0.9 * len(us))]}


def main(out):
    import torch

    import test_gpu_mlp_lean as tl
    from pnr import synth
    from pnr.renderer import NeRFRenderer

    dev = torch.device("cuda:0")
    net = tl.make_net("f16x3", True)
    sc = synth.scene_nmr(seed=3, n_rays=256)
    tl.encode_nmr(net, sc)
    rays = sc["rays"].to(dev).contiguous()
    r = NeRFRenderer(n_coarse=8, n_fine=8, white_bkgd=True).to(dev).eval()
    res = {"warmup": WARMUP, "calls": CALLS}

    def render():
        with torch.no_grad():
            r(net, rays[None])

    torch.manual_seed(3)
    res["render"] = timed(render)

    params = [p for k, p in net.named_parameters() if k.startswith("mlp_")]
    opt = torch.optim.Adam(params, lr=1e-5)
    target = torch.rand(1, 128, 3, generator=torch.Generator().manual_seed(4)).to(dev)

    def train_step():
        opt.zero_grad()
        o = r(net, rays[None, :128])
        loss = ((o.coarse.rgb - target) ** 2).mean() + ((o.fine.rgb - target) ** 2).mean()
        loss.backward()
        opt.step()

    res["train_step"] = timed(train_step)
    for k in ("render", "train_step"):
        print("%-10s median %.1f us  min %.1f  p90 %.1f" % (k, res[k]["median_us"], res[k]["min_us"], res[k]["p90_us"]),
              flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
