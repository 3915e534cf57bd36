#!/usr/bin/env python
"""Phase cycles per tile of k_point_mlp over the cfg3 (headline) render, from a PNR_PHASE_TIMING
build (PNR_LIB_PATH; -DPNR_PT_WAVE=w records wave w): tools/mlp_probe.py's table on bench.py's
cfg3 inputs (NMR 64x64, latent 32x32, 24 frames x 4096 rays x (64 + 64), mode 2).  The counters
sum every k_point_mlp launch, so the coarse pass alone is rendered too (n_fine = 0: the same coarse
tiles) and the fine launches' figures are the difference of the two.
  PNR_LIB_PATH=pixel-nerf_amd/build/pt_w0/libpnr.so python tools/phase_cfg3.py [LEAN=0|1]"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import torch  # noqa: E402
from pnr import _lib  # noqa: E402
from pnr.renderer import NeRFRenderer  # noqa: E402

SLOTS = [(8, "point_loads"), (9, "camera_geometry"), (10, "barrier_in"), (11, "pe_features_split"),
         (12, "projection"), (0, "barrier_out"), (1, "stage"), (2, "gemm"), (3, "glue_other"),
         (17, "prime_bias"), (13, "pub_colmax"), (14, "pub_barrier1"), (15, "pub_split"),
         (16, "pub_barrier2"), (4, "head")]

dev = torch.device("cuda:0")
lib = _lib.load()
dbg = getattr(lib, "pnr_debug_phase", None)
assert dbg is not None, "needs a -DPNR_PHASE_TIMING build (PNR_LIB_PATH)"
lib.pnr_render_set_fused(2)
if hasattr(lib, "pnr_mlp_set_lean"):
    lib.pnr_mlp_set_lean(int(os.environ.get("LEAN", "1")))
net = bench.make_net(dev, "f16x3", True, use_first_pool=False)
img, src, focal, rays = bench.nmr_inputs(dev)
net.encode(img, src, focal)
n_frames = int(os.environ.get("FRAMES", "6"))
chunks = list(torch.split(rays, bench.RAY_BATCH, dim=0))[:n_frames]
ph = (ctypes.c_ulonglong * 32)()


def run(n_fine):
    r = NeRFRenderer(n_coarse=64, n_fine=n_fine, white_bkgd=True, eval_batch_size=bench.RAY_BATCH).to(dev)
    with torch.no_grad():
        r(net, chunks[0][None])
        torch.cuda.synchronize()
        dbg(ph, 1)
        for c in chunks:
            r(net, c[None])
        torch.cuda.synchronize()
    dbg(ph, 0)
    return list(ph)


both, coarse = run(64), run(0)
fine = [b - c for b, c in zip(both, coarse)]
out = {"lib": os.environ.get("PNR_LIB_PATH", "default"), "lean": os.environ.get("LEAN", "1"), "frames": n_frames}
for name, v in (("coarse", coarse), ("fine", fine)):
    tiles = max(v[6], 1)
    out[name] = {"tiles": v[6], "cycles_per_tile": {nm: round(v[i] / tiles) for i, nm in SLOTS}}
    out[name]["total"] = sum(out[name]["cycles_per_tile"].values())
print(json.dumps(out))
