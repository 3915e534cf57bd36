"""Times pnr_weight_grad_arith (k_wgrad_h or k_wgrad, + k_wgrad_reduce) alone: 13 layers of 512 x 512 over P points,
the coarse training MLP's shape.  Select a libpnr.so variant with PNR_LIB_PATH; the ablation variants
(-DPNR_WG_NOPUT, -DPNR_WG_MFMA3, -DPNR_WG_L2ROWS, -DPNR_WGH_HEAD=h, -DPNR_WGH_INIT=n; results invalid) are built by
    PATCH=tools/patches/ablations.diff scripts/build_variant.sh NAME WORKTREE -D<knob>
    python tools/wgrad_probe.py [P] [jobs] [f16x3|bf16x6]"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pixel-nerf_amd"))
from pnr import train  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
J = int(sys.argv[2]) if len(sys.argv) > 2 else 13
ARITH = sys.argv[3] if len(sys.argv) > 3 else "f16x3"
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
dys = [torch.randn(P, 512, device=dev, generator=g) for _ in range(J)]
xs = [torch.relu(torch.randn(P, 512, device=dev, generator=g)) for _ in range(J)]
for _ in range(3):
    train.weight_grad(dys, xs, P, ARITH)
torch.cuda.synchronize()
n = 20
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(n):
    train.weight_grad(dys, xs, P, ARITH)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / n
fl = 2.0 * J * 512 * 512 * P
print("P=%d jobs=%d %s: %.3f ms  %.1f fp32-equivalent TFLOP/s" % (P, J, ARITH, ms, fl / ms / 1e9))
