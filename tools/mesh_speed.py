#!/usr/bin/env python
"""Times the device isosurface extraction (csrc/mcubes.hip) at the size scripts/eval.py runs it,
256^3, on one MI355X: on the density grid of the synthetic pixelNeRF net (the point query of
scripts/eval.py) and on an analytic sphere.

Per pass (HIP events around the ABI call, median of --reps after --warmup):
  count  pnr_mc_count: k_mc_count + k_mc_scan
  emit   pnr_mc_emit:  k_mc_emit_verts + k_mc_emit_faces + the 16-byte read-back of the totals
with the bytes each pass has to move at least once (grid read, edge-map write / read, outputs) and
the share of the HBM peak those bytes over the measured time come to.  Also the whole op
(allocation, the host sync on the counts, both passes), the 64 MB device-to-host copy the
skimage route needs before it can start, and the point query that produces the grid.

  python tools/mesh_speed.py [--res 256] [--out profiles/mcubes/mesh_speed.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "pixel-nerf_amd"))

import torch  # noqa: E402

from pnr import _lib, ops, synth  # noqa: E402
from pnr.models import PixelNeRFNet  # noqa: E402
from speed_common import events  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12   # bytes/s: spec peak; measured float4 copy


def _events(fn, warmup, reps):
    ms = events(fn, warmup, reps)
    return statistics.median(ms), min(ms), max(ms)


def synthetic_net(dev, negate_sigma=False):
    """The net of __graft_entry__.smoke(): synthetic weights, one SRN-like scene.  negate_sigma:
    the coarse net's sigma row negated (for a net whose sigma is negative over the whole cube)."""
    mlp = dict(type="resnet", n_blocks=5, d_hidden=512, combine_layer=3, combine_type="average")
    conf = dict(use_encoder=True, use_xyz=True, use_code=True, code=dict(num_freqs=6, freq_factor=1.5),
                use_viewdirs=True, use_code_viewdirs=False, mlp_coarse=mlp, mlp_fine=mlp,
                encoder=dict(backbone="resnet34", pretrained=False, num_layers=4))
    sc = synth.scene_srn(seed=0, n_rays=8, pick="hash")
    net = PixelNeRFNet(conf)
    sd = synth.pixelnerf_state(1)
    if negate_sigma:
        for k in ("mlp_coarse.lin_out.weight", "mlp_coarse.lin_out.bias"):
            sd[k] = sd[k].clone()
            sd[k][3] = -sd[k][3]
    net.load_state_dict(sd, strict=False)
    net = net.to(dev).eval()
    net.encode_latent(sc["latent"].to(dev), sc["poses"].to(dev), sc["focal"].to(dev), (128, 128))
    return net


def sphere(res, dev):
    ax = torch.arange(res, device=dev, dtype=torch.float64)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = (res - 1) / 2.0
    return (0.37 * res - torch.sqrt((x - c - 0.3) ** 2 + (y - c + 0.2) ** 2 + (z - c - 0.1) ** 2)).float().contiguous()


def measure(name, grid, level, warmup, reps):
    lib = _lib.load()
    dev = grid.device
    nx, ny, nz = grid.shape
    n = nx * ny * nz
    nbytes = lib.pnr_mc_workspace_bytes(nx, ny, nz)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    st = _lib.stream_of(dev)

    def count():
        _lib.check(lib.pnr_mc_count(_lib.ptr(grid), nx, ny, nz, level, _lib.ptr(ws), nbytes, _lib.ptr(counts), st),
                   "pnr_mc_count")

    count()
    n_v, n_t = counts.cpu().tolist()
    verts = torch.empty(max(n_v, 1), 3, device=dev)
    faces = torch.empty(max(n_t, 1), 3, device=dev, dtype=torch.int32)

    def emit():
        _lib.check(lib.pnr_mc_emit(_lib.ptr(grid), nx, ny, nz, level, _lib.ptr(ws), nbytes, _lib.ptr(verts), n_v,
                                   _lib.ptr(faces), n_t, st), "pnr_mc_emit")

    def whole():
        ops.marching_cubes(grid, level)

    passes = {
        "count": dict(ms=_events(count, warmup, reps), bytes=dict(grid_read=4 * n)),
        "emit": dict(ms=_events(emit, warmup, reps),
                     bytes=dict(grid_read=2 * 4 * n, edge_map_write=12 * n, edge_map_read=4 * n_v,
                                verts_write=12 * n_v, faces_write=12 * n_t)),
    }
    for p in passes.values():
        med = p["ms"][0]
        p["ms"] = dict(median=med, min=p["ms"][1], max=p["ms"][2])
        p["bytes_total"] = sum(p["bytes"].values())
        p["bytes_per_s"] = p["bytes_total"] / (med * 1e-3)
        p["share_of_hbm_spec_peak"] = p["bytes_per_s"] / HBM_SPEC
        p["share_of_hbm_measured_copy"] = p["bytes_per_s"] / HBM_COPY
    torch.cuda.synchronize(dev)
    wall = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        whole()
        torch.cuda.synchronize(dev)
        wall.append((time.perf_counter() - t0) * 1e3)
    res = dict(grid=name, shape=[nx, ny, nz], level=level, vertices=n_v, triangles=n_t, passes=passes,
               whole_op_wall_ms=statistics.median(wall[warmup:]), workspace_bytes=nbytes)
    print("%s %dx%dx%d level %g: V %d T %d" % (name, nx, ny, nz, level, n_v, n_t))
    for k, p in passes.items():
        print("  %-5s %.3f ms (min %.3f max %.3f)  %.1f MB -> %.2f TB/s = %.0f%% of the 8 TB/s spec peak, %.0f%% of "
              "the 6.29 TB/s copy rate  %s" % (k, p["ms"]["median"], p["ms"]["min"], p["ms"]["max"],
                                             p["bytes_total"] / 1e6, p["bytes_per_s"] / 1e12,
                                             100 * p["share_of_hbm_spec_peak"], 100 * p["share_of_hbm_measured_copy"],
                                             {b: round(v / 1e6, 1) for b, v in p["bytes"].items()}))
    print("  whole op (alloc + count + sync + emit), host clock: %.3f ms" % res["whole_op_wall_ms"])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_speed.py needs a HIP device: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    spec = importlib.util.spec_from_file_location("pnr_scripts_eval", os.path.join(REPO, "scripts", "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)

    out = dict(device=torch.cuda.get_device_name(0), res=args.res, hbm_spec_bytes_per_s=HBM_SPEC,
               hbm_measured_copy_bytes_per_s=HBM_COPY, runs=[])
    net = synthetic_net(dev)
    ev.density_grid(net, 32, dev)   # warm the point query
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    sig = ev.density_grid(net, args.res, dev)
    torch.cuda.synchronize(dev)
    out["point_query_s"] = time.perf_counter() - t0
    print("point query %d^3: %.3f s" % (args.res, out["point_query_s"]))
    pos = sig[sig > 0]
    if not pos.numel():   # sigma < 0 over the whole cube: the same net with its sigma row negated
        out["sigma_row_negated"] = True
        sig = ev.density_grid(synthetic_net(dev, negate_sigma=True), args.res, dev)
        pos = sig[sig > 0]
    if pos.numel():
        level = float(pos.median())
        out["runs"].append(measure("synthetic_net_density", sig, level, args.warmup, args.reps))
    else:
        print("synthetic net: the density grid is all zero, nothing to extract")
    out["runs"].append(measure("analytic_sphere", sphere(args.res, dev), 0.0, args.warmup, args.reps))

    # the copy the host route starts with: the grid to pageable host memory (.cpu()) and to pinned
    def to_host():
        sig.cpu()

    pinned = torch.empty(sig.shape, dtype=sig.dtype, pin_memory=True)
    d2h = _events(to_host, 2, 10)
    d2h_pin = _events(lambda: pinned.copy_(sig, non_blocking=True), 2, 10)
    out["grid_to_host_ms"] = dict(pageable=d2h[0], pinned=d2h_pin[0], bytes=sig.numel() * 4)
    print("grid to host (%.0f MB): %.3f ms pageable, %.3f ms pinned" % (sig.numel() * 4 / 1e6, d2h[0], d2h_pin[0]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
