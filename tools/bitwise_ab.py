#!/usr/bin/env python
"""Diagnostic (GPU): is a libpnr.so variant bit-identical to another, and as fast?
Each `save*` / `time` run uses the library PNR_LIB_PATH selects and is its own process; `cmp` runs on
the CPU.  Latents are synthetic, not a ResNet34 encode: MIOpen may pick another convolution algorithm
in another process, which changes the latent in its last bits.

  python tools/bitwise_ab.py save OUT.pt        the bench's cfg3 render: the first 8,192 rays of its batch
                                                (64 + 64, counter RNG, fixed seed): rgb, depth, weights
  python tools/bitwise_ab.py save-all OUT.pt    every k_point_mlp instantiation at the smallest shapes that
                                                exercise it (cases_all below); per case also the kernel
                                                family pnr_mlp_last_kernel names
  python tools/bitwise_ab.py cmp A.pt B.pt      bitwise equal? (torch.equal per tensor, no tolerance)
  python tools/bitwise_ab.py time OUT.json      HIP-event times of one render of 8,192 rays x (64 + 64)
                                                per instantiation no bench leg reaches: one warm-up,
                                                five repeats each (alternate the libraries by process)"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "pixel-nerf_amd"), REPO):
    sys.path.insert(0, p)

KERNEL_NAMES = {0: "none", 1: "general", 2: "lean"}


def save(out):
    import torch

    import bench
    from pnr.renderer import NeRFRenderer

    from pnr import synth

    dev = torch.device("cuda:0")
    net = bench.make_net(dev, "f16x3", True, use_first_pool=False)
    img, src, focal, rays = bench.nmr_inputs(dev)
    r = NeRFRenderer(n_coarse=bench.KC, n_fine=bench.KF, white_bkgd=True).to(dev)
    with torch.no_grad():
        net.encode_latent(synth.latent(0, 1, 512, 32, 32).to(dev), src, focal, (64, 64))
        torch.manual_seed(7)
        d = r(net, rays[:8192][None], want_weights=True)
    torch.save({f"{p}.{k}": d[p][k].cpu() for p in ("coarse", "fine") for k in ("rgb", "depth", "weights")}, out)
    print("saved", out, os.environ.get("PNR_LIB_PATH", "default"))


# ---- the second case set: every instantiation <PREC, PZ, MARCH, LEAN> ---------------------------
PRECISIONS = ("fp32", "bf16x6", "bf16x9", "f16x3", "f16")
RENDER_OUT = ("c_rgb", "c_depth", "c_w", "f_rgb", "f_depth", "f_w", "z_c", "z_f")


def _kernel(lib, precision, proj, march):
    """The instantiation a launch took, as far as the library tells: its arguments and the family."""
    return "%s pz=%d march=%d %s" % (precision, proj, march, KERNEL_NAMES[lib.pnr_mlp_last_kernel()])


def _encode(net, n_obj, n_views):
    """n_obj x n_views synthetic 32 x 32 latents and NMR cameras (test_gpu_mlp_lean's geometry)."""
    from pnr import synth

    import test_gpu_mlp_lean as tl

    n = n_obj * n_views
    sc = synth.scene_nmr(seed=3, n_rays=1)
    net.encode_latent(synth.latent(3, n, 512, 32, 32).to(tl.DEV),
                      synth.srn_poses([20.0 * i for i in range(n)], phi=-20.0, radius=2.7).reshape(n_obj, n_views, 4, 4)
                      .to(tl.DEV), sc["focal"].to(tl.DEV), (64, 64), num_objs=n_obj)


def cases_all():
    """Yields (name, {output name: tensor or string}).  A refused call yields its message, which must
    then be the other library's too."""
    import torch

    import test_gpu_mlp_lean as tl
    from pnr import _lib, synth

    lib = _lib.load()
    dev = tl.DEV

    def guarded(fn):
        try:
            return fn()
        except Exception as e:   # noqa: BLE001  (a refusal is a result to compare)
            return {"refused": "%s: %s" % (type(e).__name__, e)}

    # point query of 200 points per object (three full tiles and one of 8)
    for n_obj, n_views in ((1, 1), (2, 2)):
        xyz = torch.from_numpy(synth.hash_sym(77, (n_obj, 200, 3), 0.5)).to(dev)
        vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(78, (n_obj, 200, 3), 1.0)), dim=-1).to(dev)
        for proj in (True, False):
            for precision in PRECISIONS:
                if precision == "f16" and not proj:
                    continue

                def run():
                    net = tl.make_net(precision, proj)
                    _encode(net, n_obj, n_views)
                    with torch.no_grad():
                        out = net(xyz, coarse=True, viewdirs=vd)
                    torch.cuda.synchronize()
                    return {"out": out.cpu(), "kernel": _kernel(lib, precision, proj, 0)}

                yield "query obj%d ns%d %s proj%d" % (n_obj, n_views, precision, proj), guarded(run)

    # training forward (pnr_render_points with the activation save): 37 rays x K = 64; the whole
    # save buffer as words (mask words are no floats), prefilled so that unwritten rows compare too
    sc = synth.scene_nmr(seed=3, n_rays=37)
    rays37 = sc["rays"].to(dev).contiguous()
    t = torch.linspace(0.0, 1.0, 64, device=dev)
    z = (rays37[:, 6:7] + (rays37[:, 7:8] - rays37[:, 6:7]) * t).contiguous()
    for n_views in (1, 2):
        for precision in ("f16x3", "fp32"):

            def run():
                net = tl.make_net(precision, False)
                _encode(net, 1, n_views)
                desc, packed = net.mlp_coarse.packed(net.code, net.mlp_precision)
                scn = net.hip_scene()
                B, K = z.shape
                n_save = lib.pnr_point_save_floats(desc, B * K * n_views)
                sv = torch.full((n_save,), -7.0, dtype=torch.float32, device=dev)
                ws_bytes = lib.pnr_point_query_workspace_bytes(scn, B * K)
                ws = torch.zeros(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
                out = torch.full((B * K, 4), -7.0, dtype=torch.float32, device=dev)
                _lib.check(lib.pnr_render_points(scn, desc, _lib.ptr(packed), _lib.Rays(_lib.ptr(rays37), B, B),
                                                 _lib.ptr(z), K, _lib.ptr(out), _lib.ptr(sv), _lib.ptr(ws), ws_bytes,
                                                 _lib.stream_of(torch.device(dev))), "pnr_render_points")
                torch.cuda.synchronize()
                return {"out": out.cpu(), "save": sv.view(torch.int32).cpu(), "kernel": _kernel(lib, precision, 0, 0)}

            yield "train fwd ns%d %s" % (n_views, precision), guarded(run)

    # render of 37 and 300 rays x (64 + 64) on test_gpu_mlp_lean's scene: all eight outputs
    for n_rays in (37, 300):
        sc = synth.scene_nmr(seed=3, n_rays=n_rays)
        rays = sc["rays"].to(dev).contiguous()
        perm = torch.randperm(n_rays, generator=torch.Generator().manual_seed(5)).to(torch.int32)
        j = n_rays // 2   # one out-of-range entry, at a fixed point of the permutation
        perm[int((perm == j).nonzero()[0])] = perm[j]
        perm[j] = n_rays + 7
        streams = synth.rng_streams(11, n_rays, tl.KC, tl.KF, 0)
        for precision in PRECISIONS:
            for proj, n_views in ((True, 1), (False, 1), (True, 2)):
                if precision == "f16" and not proj:
                    continue
                net = tl.make_net(precision, proj)
                _encode(net, 1, n_views)
                for mode in (0, 1, 2, 3):
                    # the lean switch decides only where the lean kernel is served
                    leans = (True, False) if (proj and n_views == 1 and mode in (1, 2) and
                                              precision in ("f16x3", "f16")) else (True,)
                    for lean in leans:
                        for order in (None, perm.to(dev)):
                            for st in (None, streams):

                                def run():
                                    with _lib.lean_mlp(lean):
                                        res, _ = tl.render(net, rays, mode, st, order)
                                    d = {nm: x.cpu() if torch.is_tensor(x) else repr(x) for nm, x in zip(RENDER_OUT, res)}
                                    d["kernel"] = _kernel(lib, precision, proj, mode != 0)
                                    return d

                                yield ("render %d rays %s proj%d ns%d mode%d lean%d order%d draws%d" % (
                                    n_rays, precision, proj, n_views, mode, lean, order is not None, st is not None),
                                    guarded(run))


def save_all(out):
    import torch

    blob, kernels = {}, {}
    for name, d in cases_all():
        for k, v in d.items():
            blob["%s | %s" % (name, k)] = v
        kernels.setdefault(d.get("kernel", d.get("refused")), []).append(name)
    torch.save(blob, out)
    for k in sorted(kernels):
        print("%4d cases: %s" % (len(kernels[k]), k))
    print("saved", out, len(blob), "values", os.environ.get("PNR_LIB_PATH", "default"))


def cmp(a, b):
    import torch

    A, B = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    same = set(A) == set(B)
    for k in sorted(set(A) ^ set(B)):
        print(k, "on one side only")
    n = 0
    for k in A:
        if k not in B:
            continue
        n += 1
        if torch.is_tensor(A[k]):
            eq = torch.is_tensor(B[k]) and A[k].shape == B[k].shape and torch.equal(A[k], B[k])
        else:
            eq = A[k] == B[k]
        same &= eq
        if len(A) <= 16:
            print(k, "identical" if eq else "max|d| %.3e" % float((A[k] - B[k]).abs().max()))
        elif not eq:
            print(k, "DIFFERENT:", ("max|d| %.3e" % float((A[k].double() - B[k].double()).abs().max()))
                  if torch.is_tensor(A[k]) and torch.is_tensor(B[k]) and A[k].shape == B[k].shape else (A[k], B[k]))
    print("%d values compared" % n)
    print("BITWISE IDENTICAL" if same else "DIFFERENT")
    return 0 if same else 1


# ---- time mode ---------------------------------------------------------------------------------
# (name, precision, latent projection, source views, march mode, lean switch)
TIME_CASES = (
    ("fp32 <0,t,t,f>", "fp32", True, 1, 2, True),
    ("bf16x6 <6,t,t,f>", "bf16x6", True, 1, 2, True),
    ("bf16x9 <9,t,t,f>", "bf16x9", True, 1, 2, True),
    ("f16 general <1,t,t,f>", "f16", True, 1, 2, False),
    ("f16x3 general <3,t,t,f>", "f16x3", True, 1, 2, False),
    ("f16x3 mode 3 <3,t,t,f>", "f16x3", True, 1, 3, True),
    ("f16x3 two views <3,t,t,f>", "f16x3", True, 2, 2, True),
    ("f16x3 latent gather <3,f,t,f>", "f16x3", False, 1, 2, True),
    ("f16x3 mode 0 <3,t,f,f>", "f16x3", True, 1, 0, True),
)


def time_cases(out, n_rays=8192, repeats=5):
    import torch

    import test_gpu_mlp_lean as tl
    from pnr import _lib, synth

    lib = _lib.load()
    rays = synth.scene_nmr(seed=3, n_rays=n_rays)["rays"].to(tl.DEV).contiguous()
    res = {"lib": os.environ.get("PNR_LIB_PATH", "default"), "n_rays": n_rays, "cases": {}}
    for name, precision, proj, n_views, mode, lean in TIME_CASES:
        net = tl.make_net(precision, proj)
        _encode(net, 1, n_views)
        ms = []
        with _lib.lean_mlp(lean):
            tl.render(net, rays, mode, None, None)   # warm-up
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tl.render(net, rays, mode, None, None)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
        res["cases"][name] = {"ms": ms, "kernel": _kernel(lib, precision, proj, mode != 0)}
        print("%-32s %s  %s" % (name, " ".join("%.3f" % m for m in ms), res["cases"][name]["kernel"]), flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    sys.exit({"save": save, "save-all": save_all, "time": time_cases}[mode](sys.argv[2]))
