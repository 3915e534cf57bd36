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
  python tools/bitwise_ab.py save-train OUT.pt  the training backward through the ABI, into buffers pre-filled with a
                                                fixed pattern (train_cases below): the fused chain's dy / d_zlat /
                                                d_bias, the weight gradients in both arithmetics, one training step
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


# ---- the third case set: the training backward ---------------------------------------------------
FILL = -7.0   # every output buffer starts as this, so rows a kernel must not write compare too


def scale_moves_inputs(case, P=9000):
    """The (dY, X) of tests/test_gpu_train.py::test_weight_grad_scale_moves[case]."""
    import torch

    gen = torch.Generator(device="cpu").manual_seed(7)
    d = torch.randn(P, 512, generator=gen)
    x = torch.relu(torch.randn(P, 512, generator=gen))
    if case == "growing":
        ramp = torch.exp2(torch.linspace(-20, 20, P)).unsqueeze(1)
        d = d * ramp
        x = x * ramp.flip(0).sqrt()
    elif case == "late_channels":
        d[: P // 2, ::3] = 0.0
        x[: P // 2, 1::2] = 0.0
        x[P // 2:, 1::2] *= 1e4
    elif case == "rays":
        k = torch.arange(P)
        u = torch.rand(P // 64 + 1, generator=gen)
        d = d * torch.exp2(-30.0 * u[k // 64] * (k % 64).float() / 63.0).unsqueeze(1)
        x = torch.relu(torch.randn(P, 512, generator=gen) - 1.5)
        x[: P // 3, 5::7] = 0.0
    elif case == "huge_tiny":
        d[:, :64] *= 2.0 ** 80
        d[:, 64:128] *= 2.0 ** -60
        x[:, :32] *= 2.0 ** -60
        x[:, 32:64] *= 2.0 ** 20
    else:
        d.zero_()
        x.zero_()
    return d, x


def train_cases():
    """Yields (name, tensor), every tensor on the CPU."""
    import ctypes
    from types import SimpleNamespace

    import torch

    import test_gpu_train as tt
    from pnr import _lib, train
    from pnr.models import PixelNeRFNet

    lib = _lib.load()
    dev = tt.DEV

    def filled(*shape):
        return torch.full(shape, FILL, dtype=torch.float32, device=dev)

    # (a) pnr_mlp_backward_views on the parameter sets, save and d_o of
    # test_fused_mlp_backward_matches_torch_backward
    mark = [m for m in tt.test_fused_mlp_backward_matches_torch_backward.pytestmark if m.name == "parametrize"][0]
    for ps in mark.args[1]:
        rays_per_obj, K, ns, comb, nb = ps.values
        cs = tt.case(sb=2, rays_per_obj=rays_per_obj, kc=K, ns=ns, combine_layer=comb, n_blocks=nb)
        net = PixelNeRFNet(tt.conf(comb, nb))
        net.load_state_dict(cs["sd"], strict=False)
        net = net.to(dev)
        net.mlp_precision = "f16x3"
        net.encode_latent(cs["latent"].to(dev), cs["poses"].to(dev), cs["focal"].to(dev),
                          (cs["width"], cs["height"]), c=cs["c"].to(dev), num_objs=cs["poses"].shape[0])
        rays = cs["rays"].to(dev).reshape(-1, 8).contiguous()
        t = torch.linspace(0.0, 1.0, K, device=dev)
        z = (rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * t).contiguous()
        ctx = SimpleNamespace()
        ctx.save_for_backward = lambda *ts: setattr(ctx, "saved", ts)
        mlp = net.mlp_coarse
        with torch.no_grad():
            train.RenderPoints.forward(ctx, net, True, rays, z, net.encoder.latent_cl, *train.mlp_params(mlp))
        save = ctx.saved[3]
        P = rays.shape[0] * K
        gen = torch.Generator(device="cpu").manual_seed(7)
        d_o = (torch.randn(P, 4, generator=gen) * torch.exp2(-20.0 * torch.rand(P, 1, generator=gen))).to(dev)
        desc, packed, packed_t = mlp.packed_t(net.code, "f16x3")
        w_out = mlp.lin_out.weight.detach().float().contiguous()
        dy, sums = filled(2 * nb + 1, ns * P, 512), filled(2 * nb + 1, 512)
        dzl = filled(ns * P, 512) if len(mlp.lin_z) else None
        wsb = lib.pnr_mlp_backward_workspace_bytes(desc, P)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        _lib.check(lib.pnr_mlp_backward_views(desc, _lib.ptr(packed), _lib.ptr(packed_t), _lib.ptr(w_out),
                                              _lib.ptr(save), _lib.ptr(d_o), P, ns, _lib.ptr(dy), _lib.ptr(dzl),
                                              _lib.ptr(sums), _lib.ptr(ws), wsb, _lib.stream_of(rays.device)),
                   "pnr_mlp_backward_views")
        torch.cuda.synchronize()
        yield "chain %s | dy" % ps.id, dy.cpu()
        yield "chain %s | d_bias" % ps.id, sums.cpu()
        if dzl is not None:
            yield "chain %s | d_zlat" % ps.id, dzl.cpu()
        del dy, dzl, save

    # (b) pnr_weight_grad_arith
    def wgrad(dys, xs, P, arith):
        n = len(dys)
        dys, xs = [d.to(dev).contiguous() for d in dys], [x.to(dev).contiguous() for x in xs]
        out = filled(n, 512, 512)
        wsb = lib.pnr_weight_grad_workspace_bytes(n, P)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        _lib.check(lib.pnr_weight_grad_arith(arr(dys), arr(xs), arr(list(out)), n, P, _lib.WGRAD_ARITH[arith],
                                             _lib.ptr(ws), wsb, _lib.stream_of(out.device)), "pnr_weight_grad_arith")
        torch.cuda.synchronize()
        return out.cpu()

    for n, P in ((3, 1), (3, 33), (3, 4133), (16, 33)):   # test_weight_grad_matches_fp64's data
        gen = torch.Generator(device="cpu").manual_seed(P + n)
        dys = [torch.randn(P, 512, generator=gen) * torch.exp2(-30 + 40 * torch.rand(P, 1, generator=gen))
               for _ in range(n)]
        xs = [torch.relu(torch.randn(P, 512, generator=gen)) * torch.exp2(-8 * torch.rand(1, 512, generator=gen))
              for _ in range(n)]
        for arith in ("f16x3", "bf16x6"):
            yield "wgrad %d layers P=%d %s" % (n, P, arith), wgrad(dys, xs, P, arith)
    for case in ("growing", "late_channels", "huge_tiny", "zeros", "rays"):
        d, x = scale_moves_inputs(case)
        yield "wgrad scale_moves %s f16x3" % case, wgrad([d], [x], d.shape[0], "f16x3")

    # (c) one training step, the first case of test_training_step_gradients_match_oracle in f16x3: the
    # MLP parameter gradients and every RenderPoints.backward's d_z (d_latent is summed with atomics)
    dzs = []
    orig = train.RenderPoints.backward

    def recording(ctx, d_out):
        res = orig(ctx, d_out)
        if res[3] is not None:   # only a pass whose depths carry a gradient (the fine pass's depth samples)
            dzs.append(res[3].detach().cpu().clone())
        return res

    train.RenderPoints.backward = staticmethod(recording)
    try:
        _, g = tt.hip_grads(tt.case(), "f16x3")
    finally:
        train.RenderPoints.backward = staticmethod(orig)
    for k in sorted(g):
        if k != "latent":
            yield "step | %s" % k, g[k]
    for i, dz in enumerate(dzs):
        yield "step | d_z of backward %d" % i, dz


def save_train(out):
    import torch

    blob = dict(train_cases())
    torch.save(blob, out)
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
    sys.exit({"save": save, "save-all": save_all, "save-train": save_train, "time": time_cases}[mode](sys.argv[2]))
