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
  python tools/bitwise_ab.py save-march OUT.pt  the along-ray kernels through the ABI, outputs pre-filled likewise
                                                (march_cases below): composite, the samplers, the draws, the ray
                                                generator, the composite and point-input backward, and two renders
                                                whose fine pass reuses the coarse MLP
  python tools/bitwise_ab.py save-glue OUT.pt   the Python layer above the ABI, by names every revision of it has, so the
                                                file also runs from an older checkout against one library (glue_cases
                                                below): the training and callback renders with their gradients, point
                                                queries, the sampler / mesh / image wrappers, refusals
  python tools/bitwise_ab.py cmp A.pt B.pt      bitwise equal? (torch.equal per tensor, no tolerance)
  python tools/bitwise_ab.py time OUT.json      HIP-event times of one render of 8,192 rays x (64 + 64)
                                                per instantiation no bench leg reaches: one warm-up,
                                                five repeats each (alternate the libraries by process)
  python tools/bitwise_ab.py time-march OUT.json  HIP-event times of the two along-ray kernels no bench leg isolates:
                                                the generic k_composite (65,536 rays x 320) and k_composite_bwd
                                                (65,536 x 96 and x 256), three warm-ups and 20 launches each"""
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


# ---- the fourth case set: the along-ray kernels --------------------------------------------------
def march_cases():
    """Yields (name, tensor), every tensor on the CPU."""
    import torch

    import march_surface as ms
    import test_gpu_march_backward as tb
    import test_gpu_march_range as tr
    import test_gpu_mlp_lean as tl
    import test_gpu_parity as tgp
    from oracle import ref_cpu
    from pnr import _lib, synth, torchops
    from pnr.models import PixelNeRFNet
    from pnr.renderer import NeRFRenderer

    lib = _lib.load()
    dev = tr.DEV
    st = lambda: _lib.stream_of(torch.device(dev))   # noqa: E731
    up = lambda t: None if t is None else t.to(dev).contiguous()   # noqa: E731

    def filled(*shape):
        return torch.full(shape, FILL, dtype=torch.float32, device=dev)

    # pnr_composite
    def composite(rays, z, raw, white, want_w=True):
        B, K = z.shape
        rays, z, raw = up(rays), up(z), up(raw)
        w, rgb, d = (filled(B, K) if want_w else None), filled(B, 3), filled(B)
        _lib.check(lib.pnr_composite(_lib.ptr(z), _lib.ptr(raw), _lib.ptr(rays), B, K, int(white), _lib.ptr(w),
                                     _lib.ptr(rgb), _lib.ptr(d), st()), "pnr_composite")
        torch.cuda.synchronize()
        return {"w": w, "rgb": rgb, "depth": d}

    def each(name, d):
        for k, v in d.items():
            if v is not None:
                yield "%s | %s" % (name, k), v.cpu()

    for B, K in tr.COMPOSITE_CASES:
        for white in (True, False):
            yield from each("composite B=%d K=%d white=%d" % (B, K, white), composite(*tr.composite_inputs(B, K), white))
    for B, K in tr.NULL_WEIGHT_CASES:
        yield from each("composite no weights B=%d K=%d" % (B, K), composite(*tr.composite_inputs(B, K), True, False))
    for K in ms.COMPOSITE_KS:
        yield from each("composite opaque rows K=%d" % K, composite(*ms.composite_rows(K, 100 + K), True))

    # pnr_sample_coarse, pnr_rng_fill, pnr_gen_rays
    for B, K in ((3, 257), (2, 1024)):
        for lindisp in (False, True):
            g = torch.Generator().manual_seed(K)
            rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), 0.8), torch.full((B, 1), 1.8)], 1)
            u, z = up(torch.rand(B, K, generator=g)), filled(B, K)
            rays = up(rays)
            _lib.check(lib.pnr_sample_coarse(_lib.ptr(rays), B, K, _lib.ptr(u), int(lindisp), _lib.ptr(z), st()),
                       "pnr_sample_coarse")
            torch.cuda.synchronize()
            yield "sample_coarse B=%d K=%d lindisp=%d" % (B, K, lindisp), z.cpu()
    for stream in (_lib.RNG_U_COARSE, _lib.RNG_U_FINE, _lib.RNG_U_FINE_JIT, _lib.RNG_N_DEPTH):
        out = filled(5, 37)
        _lib.check(lib.pnr_rng_fill(1234, 3, int(stream), 5, 37, _lib.ptr(out), st()), "pnr_rng_fill")
        torch.cuda.synchronize()
        yield "rng_fill stream %d" % stream, out.cpu()
    poses = synth.srn_poses([10.0, 130.0], phi=-20.0, radius=2.7)
    for rows in (3, 4):
        p, out = up(poses[:, :rows]), filled(2 * 5 * 7, 8)
        _lib.check(lib.pnr_gen_rays(_lib.ptr(p), 2, rows, 7, 5, 9.5, 9.25, 3.4, 2.6, 0.8, 1.8, _lib.ptr(out), st()),
                   "pnr_gen_rays")
        torch.cuda.synchronize()
        yield "gen_rays pose rows %d" % rows, out.cpu()

    # pnr_sample_fine: the surface-like cases, then test_sample_fine_up_to_1024's
    def sample_fine(c):
        B, kc, kf, kfd = c["zc"].shape[0], c["kc"], c["kf"], c["kfd"]
        nf = kf - kfd
        t = {k: up(c[k]) for k in ("rays", "zc", "w", "depth", "u", "uj", "nd")}
        out = filled(B, kc + kf)
        _lib.check(lib.pnr_sample_fine(_lib.ptr(t["rays"]), B, kc, _lib.ptr(t["zc"]), _lib.ptr(t["w"]),
                                       _lib.ptr(t["depth"] if kfd > 0 else None), kf, kfd, ms.DEPTH_STD,
                                       _lib.ptr(t["u"] if nf > 0 else None), _lib.ptr(t["uj"] if nf > 0 else None),
                                       _lib.ptr(t["nd"] if kfd > 0 else None), int(c["lindisp"]), _lib.ptr(out), st()),
                   "pnr_sample_fine")
        torch.cuda.synchronize()
        return out.cpu()

    for case in ms.SAMPLER_CASES:
        yield "sample_fine surface %s" % (case,), sample_fine(ms.sampler_inputs(*case))
    mark = [m for m in tr.test_sample_fine_up_to_1024.pytestmark if m.name == "parametrize"][0]
    for kc, kf, kfd, lindisp in mark.args[1]:
        g = torch.Generator().manual_seed(kc + kf)   # the test's inputs (its draws are not moved off the cdf)
        B = 65
        rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), 0.5), torch.full((B, 1), 3.5)], 1)
        zc = ref_cpu.sample_coarse(rays, kc, torch.rand(B, kc, generator=g), lindisp)
        w = torch.rand(B, kc, generator=g) ** 4
        w[:3] = 0.0
        depth = 0.5 + 3.0 * torch.rand(B, generator=g)
        u, uj = torch.rand(B, kf - kfd, generator=g), torch.rand(B, kf - kfd, generator=g)
        nd = torch.randn(B, kfd, generator=g)
        yield "sample_fine range %s" % ((kc, kf, kfd, lindisp),), sample_fine(
            dict(rays=rays, zc=zc, w=w, depth=depth, u=u, uj=uj, nd=nd, kc=kc, kf=kf, kfd=kfd, lindisp=lindisp))

    # pnr_composite_backward: every K, each optional gradient present and absent, on the module's inputs and
    # on the opaque rows (with that module's output gradients)
    for K in tb.BWD_K:
        c = tb.composite_bwd_inputs(K, True)
        rays, z, raw = ms.composite_rows(K, 100 + K)
        rows = slice(0, ms.N_ROWS)
        opaque = dict(c, rays=rays, z=z, raw=raw, d_rgb=c["d_rgb"][rows], d_depth=c["d_depth"][rows], d_w=c["d_w"][rows])
        for what, cs in (("inputs", c), ("opaque rows", opaque)):
            for use_depth, use_w, want_dz in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
                rc, d_raw, d_z = tb.run_composite_bwd(cs, bool(use_depth), bool(use_w), bool(want_dz), prefill=FILL)
                _lib.check(rc, "pnr_composite_backward")
                name = "composite_bwd %s K=%d d_depth=%d d_weights=%d d_z=%d" % (what, K, use_depth, use_w, want_dz)
                yield name + " | d_raw", d_raw.cpu()
                if d_z is not None:
                    yield name + " | d_z", d_z.cpu()

    # pnr_points_input_backward: d_z only (d_latent is summed with float atomics)
    sd = synth.pixelnerf_state(5)
    for cname, p in sorted(tb.INPUT_CASES.items()):
        sn = tb.input_stage_scene(p["sb"], p["ns"], p["seed"])
        rays, z = tb.input_stage_rays(sn, p["rpo"], p["K"], p["seed"] + 100)
        n_points = p["sb"] * p["rpo"] * p["K"]
        g = torch.Generator().manual_seed(p["seed"] + 200)
        d_feat = up(torch.randn(p["ns"] * n_points, 64, generator=g))
        d_zlat = up(torch.randn(p["ns"] * n_points, 512, generator=g))
        net = PixelNeRFNet(tb.conf())
        net.load_state_dict(sd, strict=False)
        net = net.to(dev)
        net.encode_latent(sn["latent"].to(dev), sn["poses"].to(dev), sn["focal"].to(dev), (tb.IMG_W, tb.IMG_H),
                          c=sn["c"].to(dev), num_objs=sn["sb"])
        desc, packed = net.mlp_coarse.packed(net.code, "fp32")
        rays = up(rays.reshape(-1, 8))
        z = up(z.reshape(rays.shape[0], p["K"]))
        r = _lib.Rays(_lib.ptr(rays), rays.shape[0], p["rpo"])
        mask = up(torch.from_numpy(synth.hash_uniform(31, n_points) < 0.4).to(torch.uint8))
        for zm in (None, mask):
            d_lat, d_z = torch.zeros_like(net.encoder.latent_cl), filled(n_points)
            _lib.check(lib.pnr_points_input_backward_masked(
                net.hip_scene(), desc, _lib.ptr(packed), r, _lib.ptr(z), p["K"], _lib.ptr(d_feat), _lib.ptr(d_zlat),
                _lib.ptr(d_lat), _lib.ptr(d_z), _lib.ptr(zm), st()), "pnr_points_input_backward_masked")
            torch.cuda.synchronize()
            yield "points_input_bwd %s mask=%d | d_z" % (cname, zm is not None), d_z.cpu()

    # renders whose fine pass runs the coarse MLP (the origin-carrying sort, z_new, k_merge_raw):
    # 37 rays x (64 + 32) in march mode 0 with the coarse pack passed twice, then the 288-sample render of
    # test_render_with_288_samples_per_ray[True]
    net = tl.make_net("f16x3", True)
    _encode(net, 1, 1)
    rays = synth.scene_nmr(seed=3, n_rays=37)["rays"].to(dev).contiguous()
    desc, pc = net.hip_mlp(True)
    res = torchops.load().render_rays(*torchops.scene_args(net), torchops.desc_list(desc), pc, pc, net.hip_proj(True),
                                      net.hip_proj(True), rays, 37, 64, 32, 0, 0.01, True, False, None, None, None,
                                      None, 1234, 0, True, True, [], 0, None)
    torch.cuda.synchronize()
    for nm, x in zip(RENDER_OUT, res):
        yield "render shared 37 x (64 + 32) mode 0 | %s" % nm, x.cpu()
    kc, kf, kfd, B = 64, 224, 16, 13
    sc = synth.scene_srn(seed=4, n_rays=B, pick="hash")
    net = PixelNeRFNet(tgp.model_conf())
    net.load_state_dict(synth.pixelnerf_state(3), strict=False)
    net.mlp_precision = "f16x3"
    net.mlp_fine = None
    net = net.to(dev).eval()
    net.encode_latent(sc["latent"].to(dev), sc["poses"].to(dev), sc["focal"].to(dev), (128, 128))
    r = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True)
    r.streams = synth.rng_streams(6, B, kc, kf, kfd)
    r.return_z = True
    with torch.no_grad():
        out = r(net, sc["rays"][None].to(dev), want_weights=True)
    torch.cuda.synchronize()
    for pas in ("coarse", "fine"):
        for k in ("rgb", "depth", "weights", "z"):
            yield "render shared 288 samples | %s.%s" % (pas, k), getattr(getattr(out, pas), k).cpu()


def save_march(out):
    import torch

    blob = dict(march_cases())
    torch.save(blob, out)
    print("saved", out, len(blob), "values", os.environ.get("PNR_LIB_PATH", "default"))


# ---- the fifth case set: the Python layer above the ABI ----------------------------------------------
# (n_coarse, n_fine, n_fine_depth); the last is a fine pass over the coarse samples (using_fine, n_fine set to 0)
GLUE_SAMPLES = ((8, 6, 2), (8, 2, 2), (8, 6, 0), (8, 0, 0))


def glue_cases():
    """Yields (name, tensor or string): the paths of the Python layer that the other sets do not reach, through
    names every revision of it has.  37 rays, one and two source views, a 32 x 32 synthetic latent.  A refused call
    yields its exception's class and text; where the text is this layer's own wording of a library refusal, the class
    alone ("refused class")."""
    import numpy as np
    import torch

    import mc_ref
    import mesh_ref
    import meshclean_ref
    import raster_ref
    import test_gpu_mlp_lean as tl
    import test_gpu_parity as tgp
    from pnr import _lib, encoder, ops, synth, util
    from pnr.models import PixelNeRFNet, ResnetFC
    from pnr.renderer import NeRFRenderer

    dev = torch.device("cuda:0")
    rays37 = synth.scene_nmr(seed=3, n_rays=37)["rays"].to(dev).contiguous()

    def refusal(fn, text=True):
        try:
            fn()
        except Exception as e:   # noqa: BLE001  (a refusal is a result to compare)
            return "%s: %s" % (type(e).__name__, e) if text else type(e).__name__
        return "not refused"

    def encode(net, ns):
        """One object of ns views; the latent is a leaf, so its gradient is a result."""
        lat = synth.latent(3, ns, 512, 32, 32).to(dev).requires_grad_(True)
        poses = synth.srn_poses([20.0 * i for i in range(ns)], phi=-20.0, radius=2.7).reshape(1, ns, 4, 4)
        net.encode_latent(lat, poses.to(dev), synth.scene_nmr(seed=3, n_rays=1)["focal"].to(dev), (64, 64), num_objs=1)
        return lat

    def renderer(samples, noise):
        kc, kf, kfd = samples
        r = NeRFRenderer(n_coarse=kc, n_fine=max(kf, 1), n_fine_depth=kfd, noise_std=noise, white_bkgd=True).to(dev)
        r.n_fine = kf   # (8, 0, 0): using_fine stays set
        r.return_z = True
        return r.train()

    def rendered(name, net, lat, r, grad):
        """The outputs of one render under torch.manual_seed and, with ``grad``, the gradients of a fixed scalar."""
        torch.manual_seed(13)
        with torch.enable_grad() if grad else torch.no_grad():
            out = r(net, rays37[None], want_weights=True)
        loss = 0.0
        for p in ("coarse", "fine"):
            for k, wgt in (("rgb", 1.0), ("depth", 0.5), ("weights", 0.25), ("z", None)):
                t = out[p][k]
                yield "%s | %s.%s" % (name, p, k), t.detach().cpu()
                if wgt is not None:   # a ramp per element: the gradient that reaches the composite is a dense tensor
                    loss = loss + (t * torch.linspace(wgt, 2.0 * wgt, t.numel(), device=dev).reshape(t.shape)).sum()
        if grad:
            yield from grads(name, net, lat, loss)

    def grads(name, net, lat, loss):
        net.zero_grad()
        lat.grad = None
        loss.backward()
        torch.cuda.synchronize()
        for k, p in net.named_parameters():
            if k.startswith("mlp_"):
                yield "%s | d %s" % (name, k), (p.grad.cpu() if p.grad is not None else "no gradient")
        yield "%s | d latent (atomic scatter)" % name, (lat.grad.cpu() if lat.grad is not None else "no gradient")

    # (a) NeRFRenderer._forward_train: the fused conf with trainable parameters, training mode
    for ns in (1, 2):
        net = tl.make_net("f16x3", True)
        lat = encode(net, ns)
        for samples in GLUE_SAMPLES:
            for noise in (0.0, 0.5):
                yield from rendered("train ns%d %s noise %.1f" % (ns, samples, noise), net, lat, renderer(samples, noise),
                                    True)

    # (b) NeRFRenderer._forward_callback: a conf the fused kernel refuses (use_code_viewdirs), on its initial weights
    cf = tgp.model_conf()
    cf["use_code_viewdirs"] = True
    for ns in (1, 2):
        torch.manual_seed(0)
        net = PixelNeRFNet(cf).to(dev).eval()
        yield "callback ns%d | why not fused" % ns, str(net.fused_conf_reason())
        lat = encode(net, ns)
        for samples in GLUE_SAMPLES:
            for noise in (0.0, 0.5):
                for grad in (True, False):
                    yield from rendered("callback ns%d %s noise %.1f grad%d" % (ns, samples, noise, grad), net, lat,
                                        renderer(samples, noise), grad)

    # (c) PixelNeRFNet.forward as a point query of 200 points: no_grad, autograd, xyz.requires_grad
    for ns in (1, 2):
        net = tl.make_net("f16x3", True)
        lat = encode(net, ns)
        xyz = torch.from_numpy(synth.hash_sym(77, (1, 200, 3), 0.5)).to(dev)
        vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(78, (1, 200, 3), 1.0)), dim=-1).to(dev)
        for coarse in (True, False):
            name = "query ns%d coarse%d" % (ns, coarse)
            with torch.no_grad():
                yield name + " no_grad | out", net(xyz, coarse=coarse, viewdirs=vd).cpu()
            out = net(xyz, coarse=coarse, viewdirs=vd)
            yield name + " autograd | out", out.detach().cpu()
            yield from grads(name + " autograd", net, lat, (out * out).sum())
            x = xyz.clone().requires_grad_(True)
            out = net(x, coarse=coarse, viewdirs=vd)
            yield name + " xyz.requires_grad | out", out.detach().cpu()
            yield from grads(name + " xyz.requires_grad", net, lat, (out * out).sum())
            yield name + " xyz.requires_grad | d xyz", x.grad.cpu()

    # (d) the sampler and composite wrappers, the draws, the ray generator, the channels-last latent
    g = torch.Generator().manual_seed(9)
    u_c, u_f, u_j, n_d = (t.to(dev) for t in synth.rng_streams(5, 37, 8, 6, 2))
    z_c = ops.sample_coarse(rays37, 8, u_c, False)
    raw = torch.rand(37, 8, 4, generator=g).to(dev)
    w, rgb, depth = ops.composite(z_c, raw, rays37, True)
    yield "sample_coarse", z_c.cpu()
    for k, t in (("weights", w), ("rgb", rgb), ("depth", depth)):
        yield "composite | %s" % k, t.cpu()
    yield "composite no weights | rgb", ops.composite(z_c, raw, rays37, False, want_weights=False)[1].cpu()
    yield "sample_fine", ops.sample_fine(rays37, z_c, w, depth, 6, 2, 0.01, u_f, u_j, n_d, False).cpu()
    yield "sample_fine lindisp no depth", ops.sample_fine(rays37, z_c, w, depth, 4, 0, 0.01, u_f, u_j, None, True).cpu()
    yield "rng_fill", ops.rng_fill(1234, 3, _lib.RNG_U_FINE, 5, 37, dev).cpu()
    yield "gen_rays", util.gen_rays(synth.srn_poses([10.0, 130.0], phi=-20.0, radius=2.7).to(dev), 7, 5,
                                    torch.tensor([9.5, 9.25]), 0.8, 1.8, c=torch.tensor([3.4, 2.6])).cpu()
    for nhwc in (True, False):
        maps = [torch.randn(2, c, h, h, generator=g).to(dev) for c, h in ((5, 8), (3, 4), (4, 2))]
        if nhwc:
            maps = [t.contiguous(memory_format=torch.channels_last) for t in maps]
        maps = [t.requires_grad_(True) for t in maps]
        out = encoder.LatentChannelsLast.apply(*maps)
        yield "latent_channels_last nhwc%d | out" % nhwc, out.detach().cpu()
        (out * torch.randn(out.shape, generator=g).to(dev)).sum().backward()
        for i, t in enumerate(maps):
            yield "latent_channels_last nhwc%d | d map %d" % (nhwc, i), t.grad.contiguous().cpu()

    # (e) the mesh and image wrappers, one call each
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    verts, faces = ops.marching_cubes(up(mc_ref.sphere_grid((9, 8, 7), (4.2, 3.6, 3.1), 2.4)), 0.0)
    yield "marching_cubes | verts", verts.cpu()
    yield "marching_cubes | faces", faces.cpu()
    x, y = torch.rand(2, 23, 29, 3, generator=g).to(dev), torch.rand(2, 23, 29, 3, generator=g).to(dev)
    for k, t in zip(("psnr", "ssim"), ops.image_metrics(x, y)):
        yield "image_metrics | %s" % k, t.cpu()
    v, f = (up(a) for a in mesh_ref.icosphere(1, 0.8))
    for k, t in zip(("points", "normals", "tri", "area"), ops.mesh_sample(v, f, 100, seed=7)):
        yield "mesh_sample | %s" % k, t.cpu()
    pts = ops.box_sample((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 150, seed=3, device=dev)
    yield "box_sample", pts.cpu()
    for k, t in zip(("d2", "idx"), ops.nearest(pts, v)):
        yield "nearest | %s" % k, t.cpu()
    yield "winding_number", ops.winding_number(v, f, pts).cpu()
    rv, rf = (up(a) for a in raster_ref.sphere_with_floater(1))
    poses = up(raster_ref.golden_poses(2, 1.3))
    face, depth = ops.mesh_raster(rv, rf, poses, 16, 16, 16.4, c=8.0)
    yield "mesh_raster | face", face.cpu()
    yield "mesh_raster | depth", depth.cpu()
    rgb, normal = ops.mesh_shade(rv, rf, poses, 16, 16, 16.4, face, depth, c=8.0, lights=((2.0, 1.0, 3.0),),
                                 weights=(0.7,), want_normal=True)
    yield "mesh_shade | rgb", rgb.cpu()
    yield "mesh_shade | normal", normal.cpu()
    yield "mesh_shade no lights | rgb", ops.mesh_shade(rv, rf, poses, 16, 16, 16.4, face, depth, c=8.0)[0].cpu()
    sv, sf = (up(a) for a in meshclean_ref.soup(*mesh_ref.icosphere(1, 0.8)))
    for k, t in zip(("verts", "faces", "remap"), ops.mesh_weld(sv, sf)):
        yield "mesh_weld | %s" % k, t.cpu()
    vl, fl, n_c = ops.mesh_components(rv, rf)
    yield "mesh_components | vert_label", vl.cpu()
    yield "mesh_components | face_label", fl.cpu()
    yield "mesh_components | count", str(n_c)
    for k, t in sorted(ops.mesh_component_stats(rv, rf, vl, fl).items()):
        yield "mesh_component_stats | %s" % k, t.cpu()

    # (f) refusals: a size the library refuses (no launch), and arguments this layer refuses
    yield "refused marching_cubes 1025", refusal(lambda: ops.marching_cubes(torch.zeros(1025, 1, 1, device=dev), 0.0))
    yield "refused image_metrics 8193", refusal(lambda: ops.image_metrics(torch.zeros(1, 8193, 7, 1, device=dev),
                                                                          torch.zeros(1, 8193, 7, 1, device=dev)))
    yield "refused mesh_raster 8193", refusal(lambda: ops.mesh_raster(rv, rf, poses, 8193, 1, 16.4))
    yield "refused sample_coarse cpu", refusal(lambda: ops.sample_coarse(rays37.cpu(), 8, u_c))
    yield "refused composite float64", refusal(lambda: ops.composite(z_c.double(), raw, rays37, True))
    yield "refused box_sample cpu", refusal(lambda: ops.box_sample((0, 0, 0), (1, 1, 1), 4, device="cpu"))
    yield "refused mesh_shade lights", refusal(lambda: ops.mesh_shade(rv, rf, poses, 16, 16, 16.4, face, depth,
                                                                      lights=((1.0, 2.0),), weights=(1.0,)))
    net = tl.make_net("fp32", True)
    encode(net, 1)
    yield "refused render cpu rays", refusal(lambda: renderer((8, 6, 2), 0.0)(net, rays37[None].cpu()))
    narrow = ResnetFC(42, d_latent=256, d_hidden=256).to(dev)
    yield "refused class pack of a 256-wide MLP", refusal(lambda: narrow.packed(net.code, "fp32"), text=False)
    yield "refused class transposed pack in fp32", refusal(lambda: net.mlp_coarse.packed_t(net.code, "fp32"), text=False)


def save_glue(out):
    import torch

    blob = dict(glue_cases())
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
            print(k, "DIFFERENT:", ("max|d| %.3e of max|a| %.3e" % (float((A[k].double() - B[k].double()).abs().max()),
                                                                    float(A[k].double().abs().max())))
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


def time_march(out, n_rays=65536, warmup=3, launches=20):
    import torch

    from pnr import _lib

    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    res = {"lib": os.environ.get("PNR_LIB_PATH", "default"), "n_rays": n_rays, "cases": {}}

    def timed(name, call):
        ms = []
        for i in range(warmup + launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(call(), name)
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
        res["cases"][name] = {"ms": ms, "median_ms": sorted(ms)[len(ms) // 2]}
        print("%-28s median %.4f ms  min %.4f  max %.4f" % (name, res["cases"][name]["median_ms"], min(ms), max(ms)),
              flush=True)

    # (the backward at K = 256 too: k_composite_bwd<4> is the instantiation nearest a VGPR occupancy step)
    for name, K in (("k_composite 65536 x 320", 320), ("k_composite_bwd 65536 x 96", 96),
                    ("k_composite_bwd 65536 x 256", 256)):
        near, far = 0.3, 4.0
        rays = torch.cat([torch.randn(n_rays, 6, generator=g), torch.full((n_rays, 1), near),
                          torch.full((n_rays, 1), far)], 1).to(dev)
        z = torch.sort(near + (far - near) * torch.rand(n_rays, K, generator=g), -1)[0].to(dev)
        raw = torch.rand(n_rays, K, 4, generator=g)
        raw[..., 3] = torch.randn(n_rays, K, generator=g) * 4.0
        raw = raw.to(dev)
        st = _lib.stream_of(dev)
        if K > 256:
            w, rgb, d = (torch.empty(n_rays, K, device=dev), torch.empty(n_rays, 3, device=dev),
                         torch.empty(n_rays, device=dev))
            timed(name, lambda: lib.pnr_composite(_lib.ptr(z), _lib.ptr(raw), _lib.ptr(rays), n_rays, K, 1, _lib.ptr(w),
                                                  _lib.ptr(rgb), _lib.ptr(d), st))
        else:
            d_rgb, d_depth = torch.randn(n_rays, 3, generator=g).to(dev), torch.randn(n_rays, generator=g).to(dev)
            d_w = torch.randn(n_rays, K, generator=g).to(dev)
            d_raw, d_z = torch.empty(n_rays, K, 4, device=dev), torch.empty(n_rays, K, device=dev)
            timed(name, lambda: lib.pnr_composite_backward(_lib.ptr(z), _lib.ptr(raw), _lib.ptr(rays), n_rays, K, 1,
                                                           _lib.ptr(d_rgb), _lib.ptr(d_depth), _lib.ptr(d_w),
                                                           _lib.ptr(d_raw), _lib.ptr(d_z), st))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    sys.exit({"save": save, "save-all": save_all, "save-train": save_train, "save-march": save_march,
              "save-glue": save_glue, "time": time_cases, "time-march": time_march}[mode](sys.argv[2]))
