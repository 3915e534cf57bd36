"""The "f16" render mode (PNR_PREC_F16: one fp16 product per k-step in the 512 -> 512 layers) on an
MI355X (``-m gpu``).

The mode is not fp32-accurate by design, so its yardstick is the CPU emulation of its arithmetic
(tests/f16_emul.py).  In this file

    ref = the unpatched oracle,   emu = the oracle on the emulation,   hip = the GPU in "f16".

An output group is *bounded by the emulation* when

    |hip - ref| <= 2 max|emu - ref| + (5e-5 + 1e-5 |ref|)        elementwise, and
    0.5 <= mean|hip - ref| / mean|emu - ref| <= 1.5              on rgb.

hip and emu round the same operands at the same scales, so their errors are one population up to
the accumulation order; two draws of a maximum over ~10^3 values differ by well under 2x; a kernel
that loses a bit (wrong exponent, subnormal operands) doubles the mean; one that still runs three
products sends the ratio to ~0.  The fine pass is compared at hip's OWN fine samples: importance
sampling is a discontinuous function of the coarse weights, and weights that differ by 1e-4 draw
other samples on a fifth of the rays (the sampler's discontinuity, not an error)."""
import functools

import pytest
import torch

import f16_emul
import fixtures
import test_gpu_parity as tgp
from oracle import parity, ref_cpu
from pnr import synth, util
from pnr.models import PixelNeRFNet
from pnr.renderer import NeRFRenderer

pytestmark = pytest.mark.gpu

DEV = "cuda"
ATOL, RTOL = f16_emul.ATOL, f16_emul.RTOL


def with_emulation(fn):
    """fn() with ref_cpu.resnetfc_forward replaced by the emulation."""
    with pytest.MonkeyPatch.context() as mp:
        f16_emul.install(mp)
        with torch.no_grad():
            return fn()


def bounded(hip, ref, emu, name, atol=ATOL):
    """|hip - ref| <= 2 max|emu - ref| + (atol + 1e-5 |ref|), elementwise; figures printed first."""
    hip, ref, emu = [t.detach().double().cpu().reshape(-1) for t in (hip, ref, emu)]
    assert hip.shape == ref.shape == emu.shape, (name, hip.shape, ref.shape, emu.shape)
    dh = (hip - ref).abs()
    ee = float((emu - ref).abs().max())
    print("f16 %-28s max|hip-ref| %.3e  max|emu-ref| %.3e" % (name, float(dh.max()), ee))
    bad = dh > 2.0 * ee + atol + RTOL * ref.abs()
    assert not bool(bad.any()), "%s: %d/%d outside 2 x max|emu - ref| (%.3e) + fp32 term; max|hip - ref| %.3e" % (
        name, int(bad.sum()), bad.numel(), ee, float(dh.max()))


def mean_ratio(hip, ref, emu, name):
    hip, ref, emu = [t.detach().double().cpu().reshape(-1) for t in (hip, ref, emu)]
    mh, me = float((hip - ref).abs().mean()), float((emu - ref).abs().mean())
    r = mh / me if me > 0 else float("inf")
    print("f16 %-28s mean|hip-ref| %.3e  mean|emu-ref| %.3e  ratio %.3f" % (name, mh, me, r))
    assert 0.5 <= r <= 1.5, "%s: mean error ratio hip / emu = %.3f outside [0.5, 1.5]" % (name, r)


def bounded_raw(hip, ref, emu, name, atol=ATOL):
    """A (.., 4) model output: rgb and sigma as two groups, the mean ratio on rgb."""
    bounded(hip[..., :3], ref[..., :3], emu[..., :3], name + " rgb", atol)
    bounded(hip[..., 3], ref[..., 3], emu[..., 3], name + " sigma", atol)
    mean_ratio(hip[..., :3], ref[..., :3], emu[..., :3], name + " rgb")


def f16_net(sd, lat, poses, focal, wh, c=None, num_objs=1, precision="f16"):
    net = PixelNeRFNet(tgp.model_conf())
    net.mlp_precision = precision
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected
    net = net.to(DEV).eval()
    net.encode_latent(lat.to(DEV), poses.to(DEV), focal.to(DEV), wh, c=None if c is None else c.to(DEV),
                      num_objs=num_objs)
    return net


# ---- 1. point queries -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pointquery_refs():
    cfg, arr = fixtures.load("fw_pointquery")
    sd = fixtures.state_dict(cfg)
    scene = ref_cpu.Scene(fixtures.latent_of(cfg), arr["poses"], fixtures.focal_of(arr), cfg["width"],
                          cfg["height"], None)
    xyz, vd = arr["xyz"], torch.zeros_like(arr["xyz"])
    with torch.no_grad():
        ref = [ref_cpu.pixelnerf_forward(sd, scene, xyz, c, vd) for c in (True, False)]
    emu = with_emulation(lambda: [ref_cpu.pixelnerf_forward(sd, scene, xyz, c, vd) for c in (True, False)])
    return cfg, arr, ref, emu


def test_point_query_fixture_bounded_by_emulation():
    """fw_pointquery: 512 points (8 full tiles), the coarse and the fine MLP."""
    cfg, arr, ref, emu = pointquery_refs()
    net = tgp.hip_net(dict(cfg, n_blocks=5, combine_layer=3, with_fine=True, d_latent=512, d_hidden=512),
                      arr, "f16")
    with torch.no_grad():
        vd = torch.zeros_like(arr["xyz"]).to(DEV)
        oc = net(arr["xyz"].to(DEV), coarse=True, viewdirs=vd)
        of = net(arr["xyz"].to(DEV), coarse=False, viewdirs=vd)
    bounded_raw(oc, ref[0], emu[0], "pointquery coarse")
    bounded_raw(of, ref[1], emu[1], "pointquery fine")


def test_point_query_multiview_multiobject_bounded_by_emulation():
    """SB = 2 objects x NS = 3 views, P = 200 (a partial tile), per-object focal / c: the
    multi-view sum and the per-(view, point) column scales."""
    sb, ns, P = 2, 3, 200
    sd = synth.pixelnerf_state(4)
    lat = synth.latent(9, sb * ns, 512, 12, 16)
    poses = synth.srn_poses([-20.0 + 15 * i for i in range(sb * ns)], radius=1.6).reshape(sb, ns, 4, 4)
    focal = torch.tensor([[60.0, 64.0], [70.0, 66.0]])
    c = torch.tensor([[31.0, 30.0], [33.0, 29.0]])
    xyz = torch.from_numpy(synth.hash_sym(77, (sb, P, 3), 0.5))
    vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(78, (sb, P, 3), 1.0)), dim=-1)
    scene = ref_cpu.Scene(lat, poses, focal, 64, 60, c)
    with torch.no_grad():
        ref = ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd)
    emu = with_emulation(lambda: ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd))
    net = f16_net(sd, lat, poses, focal, (64, 60), c, sb)
    with torch.no_grad():
        out = net(xyz.to(DEV), coarse=True, viewdirs=vd.to(DEV))
    bounded_raw(out, ref, emu, "SB=2 NS=3")


# ---- 2. dynamic range -------------------------------------------------------------------------
def _range_scene(lat_scale=1.0, w_scale=1.0):
    sd = synth.pixelnerf_state(5)
    for k in list(sd):
        if ".lin_z." in k and k.endswith("weight"):
            sd[k] = sd[k] * w_scale
    lat = synth.latent(11, 1, 512, 16, 16) * lat_scale
    poses = synth.srn_poses([10.0])
    focal = torch.tensor(40.0)
    xyz = torch.from_numpy(synth.hash_sym(91, (1, 300, 3), 0.5))
    vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(92, (1, 300, 3), 1.0)), dim=-1)
    return sd, lat, poses, focal, xyz, vd


@pytest.mark.parametrize("lat_scale,w_scale", [(1e-4, 1.0), (1e3, 1.0), (1.0, 1e-3), (0.0, 1.0)])
def test_point_query_dynamic_range_bounded_by_emulation(lat_scale, w_scale):
    """The power-of-two column / layer scales keep the single-product mode at its own error level
    when the latent or the lin_z weights are far from unit scale, and on an all-zero latent.  The
    fp32 term is relative to the output's magnitude, as in the fp32-accurate modes' test."""
    sd, lat, poses, focal, xyz, vd = _range_scene(lat_scale, w_scale)
    scene = ref_cpu.Scene(lat, poses, focal, 64, 64, None)
    with torch.no_grad():
        ref = ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd)
    emu = with_emulation(lambda: ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd))
    net = f16_net(sd, lat, poses, focal, (64, 64))
    with torch.no_grad():
        out = net(xyz.to(DEV), coarse=True, viewdirs=vd.to(DEV)).cpu()
    assert torch.isfinite(out).all()
    mag = float(ref.abs().max())
    name = "lat*%g w*%g" % (lat_scale, w_scale)
    atol = ATOL * max(1.0, mag)
    bounded(out[..., :3], ref[..., :3], emu[..., :3], name + " rgb", atol)
    bounded(out[..., 3], ref[..., 3], emu[..., 3], name + " sigma", atol)
    # sigma is the unsaturated output of the same operands: its ratio is asserted in every case
    mean_ratio(out[..., 3], ref[..., 3], emu[..., 3], name + " sigma")
    # the rgb ratio compares two populations of errors.  With the latent x 1000 the sigmoid
    # saturates (pre-activations in the thousands) and ONE of the 900 rgb values carries the whole
    # mean; a 1-ulp fp32 perturbation of the latent moves that "mean" of the emulation itself by
    # 0.59x .. 1x (measured on the CPU), more than the margin.  The rule, from ref and emu alone:
    # the rgb ratio is asserted unless a single element holds more than a tenth of sum|emu - ref|.
    d = (emu[..., :3] - ref[..., :3]).abs()
    if float(d.max()) <= 0.1 * float(d.sum()):
        mean_ratio(out[..., :3], ref[..., :3], emu[..., :3], name + " rgb")
    else:
        assert (lat_scale, w_scale) == (1e3, 1.0), "only the saturated case may skip the rgb ratio"
        print("f16 %s rgb: one element holds %.0f %% of sum|emu - ref|; ratio asserted on sigma" % (
            name, 100.0 * float(d.max()) / float(d.sum())))


def test_point_query_nan_point_stays_confined():
    """NaN view directions on 3 points of 3 different tiles: those points are NaN (a NaN column
    maximum leaves the column unscaled, and fp16 keeps the NaN), no other point is affected."""
    sd, lat, poses, focal, xyz, vd = _range_scene()
    bad = [5, 70, 200]
    vd[0, bad] = float("nan")
    scene = ref_cpu.Scene(lat, poses, focal, 64, 64, None)
    with torch.no_grad():
        ref = ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd)
    emu = with_emulation(lambda: ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd))
    net = f16_net(sd, lat, poses, focal, (64, 64))
    with torch.no_grad():
        out = net(xyz.to(DEV), coarse=True, viewdirs=vd.to(DEV)).cpu()
    good = torch.ones(300, dtype=torch.bool)
    good[bad] = False
    assert bool(torch.isnan(ref[0, bad]).all()) and bool(torch.isnan(emu[0, bad]).all())
    assert bool(torch.isnan(out[0, bad]).all())
    assert bool(torch.isfinite(out[0, good]).all())
    bounded_raw(out[0, good], ref[0, good], emu[0, good], "beside NaN points")


# ---- 3. renders -------------------------------------------------------------------------------
def _coarse_only(sd, scene, kw, cfg, arr):
    streams = (arr["u_coarse"], arr["u_fine"], arr["u_fine_jit"], arr["n_depth"])
    return ref_cpu.render(lambda p, c, d: ref_cpu.pixelnerf_forward(sd, scene, p, c, d, **kw), arr["rays"],
                          cfg["n_coarse"], 0, 0, streams, cfg["white_bkgd"], cfg["lindisp"],
                          using_fine=False)["coarse"]


@pytest.mark.parametrize("name", ["fw_cfg3_nmr", "fw_dtu_ns3", "fw_shipped"])
def test_render_fixture_bounded_by_emulation(name):
    """fw_cfg3_nmr (128 rays, 64 + 64), fw_dtu_ns3 (64 rays, NS = 3), fw_shipped (64 + 32 with 16
    depth samples: K = 96 ends in a half tile); injected streams.  No ray is excluded anywhere."""
    cfg, arr = fixtures.load(name)
    sd, scene, kw, white, rpo = tgp.fixture_oracle(cfg, arr)
    out = tgp.hip_render(cfg, arr, precision="f16")
    c, f = out.coarse, out.fine
    B = arr["rays"].reshape(-1, 8).shape[0]
    # coarse pass: the sampler is fp32 and unchanged, so z is the streams' own
    with torch.no_grad():
        ref_c = _coarse_only(sd, scene, kw, cfg, arr)
    emu_c = with_emulation(lambda: _coarse_only(sd, scene, kw, cfg, arr))
    tgp.assert_close(c.z.reshape(B, -1), ref_c["z"].reshape(B, -1), name + " z_coarse", atol=2e-6, rtol=2e-6)
    for k in ("rgb", "depth", "weights"):
        bounded(c[k], ref_c[k], emu_c[k], "%s coarse %s" % (name, k))
    mean_ratio(c.rgb, ref_c["rgb"], emu_c["rgb"], name + " coarse rgb")
    # fine samples: every ray's z_fine is the reference algorithm's draw from hip's own coarse outputs
    streams = (arr["u_coarse"], arr["u_fine"], arr["u_fine_jit"], arr["n_depth"])
    z_sets = parity.expected_fine_sets(arr["rays"], c.z, c.weights, c.depth, streams, c.z.shape[-1],
                                       cfg["n_fine"], cfg.get("n_fine_depth", 0), cfg.get("depth_std", 0.01),
                                       cfg.get("lindisp", False))
    zh = f.z.reshape(B, -1).float().cpu()
    follows = torch.zeros(B, dtype=torch.bool)
    for ze in z_sets:
        follows |= parity.close_mask(zh, ze.reshape(B, -1)).all(-1)
    assert bool(follows.all()), "%s: rays %s do not draw their fine samples from their own coarse outputs" % (
        name, torch.nonzero(~follows).reshape(-1).tolist())
    # fine outputs on every 4th ray against the oracle fine pass at hip's own samples
    idx = list(range(0, B, 4))
    with torch.no_grad():
        w_r, rgb_r, d_r = parity.fine_pass_at(sd, scene, arr["rays"], f.z, idx, rpo, white, kw)
    w_e, rgb_e, d_e = with_emulation(lambda: parity.fine_pass_at(sd, scene, arr["rays"], f.z, idx, rpo, white, kw))
    sel = torch.tensor(idx)
    bounded(f.rgb.reshape(B, 3).cpu()[sel], rgb_r, rgb_e, name + " fine rgb")
    bounded(f.depth.reshape(B).cpu()[sel], d_r, d_e, name + " fine depth")
    bounded(f.weights.reshape(B, -1).cpu()[sel], w_r, w_e, name + " fine weights")
    mean_ratio(f.rgb.reshape(B, 3).cpu()[sel], rgb_r, rgb_e, name + " fine rgb")


# ---- 4. schedules -----------------------------------------------------------------------------
def _march_scene(n_views, sb, n_rays=130):
    """The synthetic scenes of test_fused_march_matches_unfused at 130 rays (two full 64-ray groups
    and a remainder)."""
    if n_views == 1 and sb == 1:
        sc = synth.scene_srn(seed=5, n_rays=n_rays, pick="all")
        return sc["latent"], sc["poses"], sc["focal"], (128, 128), sc["rays"].reshape(1, -1, 8)
    lat = synth.latent(10, sb * n_views, 512, 30, 40)
    poses = synth.srn_poses([30.0 * i for i in range(sb * n_views)], radius=1.4).reshape(sb, n_views, 4, 4)
    focal = torch.tensor(90.0)
    rays = util.gen_rays(synth.srn_poses([15.0 + 40.0 * i for i in range(sb)], radius=1.4), 96, 80,
                         focal, 0.4, 2.4).reshape(sb, -1, 8)
    idx = torch.from_numpy((synth.hash_uniform(3, n_rays) * rays.shape[1]).astype("int64"))
    return lat, poses, focal, (96, 80), rays[:, idx].contiguous()


@pytest.mark.parametrize("kc,kf,kfd,n_views,sb", [(64, 64, 0, 1, 1), (64, 32, 16, 1, 1), (32, 32, 0, 1, 1),
                                                  (64, 64, 16, 3, 2)])
def test_march_modes_and_ray_order_bit_identical(kc, kf, kfd, n_views, sb):
    """March modes 1, 2, 3 are bit-identical to the separate kernels (mode 0) in "f16", with and
    without return_z; on the first row the blocked ray order is bit-identical to the input order."""
    lat, poses, focal, wh, rays = _march_scene(n_views, sb)
    net = f16_net(synth.pixelnerf_state(1), lat, poses, focal, wh, None, sb)
    r = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, depth_std=0.01, white_bkgd=sb == 1)
    rays = rays.to(DEV)

    def run(mode, return_z, order="input"):
        r.march_mode, r.return_z, r.ray_order = mode, return_z, order
        with torch.no_grad():
            torch.manual_seed(11)
            return r(net, rays, want_weights=True)

    for return_z in (True, False):
        base = run(0, return_z)
        keys = ("rgb", "depth", "weights") + (("z",) if return_z else ())
        for mode in (1, 2, 3):
            o = run(mode, return_z)
            for p in ("coarse", "fine"):
                assert ("z" in o[p]) == return_z
                for k in keys:
                    assert torch.equal(o[p][k], base[p][k]), (mode, return_z, p, k,
                                                              float((o[p][k] - base[p][k]).abs().max()))
        if (kc, kf, kfd, n_views, sb) == (64, 64, 0, 1, 1):
            # 130 rays are fewer than four 16 x 16 blocks (ray_block_order then keeps the input
            # order), so the blocks are 4 x 4 here: a real permutation of the scheduling units
            from pnr import renderer as rmod

            small = functools.partial(rmod.ray_block_order, block=4)
            order = small(rays[0])
            assert order is not None and not torch.equal(order.cpu(), torch.arange(rays.shape[1], dtype=torch.int32))
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(rmod, "ray_block_order", small)
                for mode in (1, 2, 3):
                    o = run(mode, return_z, "blocked")
                    for p in ("coarse", "fine"):
                        for k in keys:
                            assert torch.equal(o[p][k], base[p][k]), ("blocked", mode, return_z, p, k)
    torch.cuda.synchronize()
    w = base.coarse.weights
    assert bool((w >= 0).all()) and float(w.sum(-1).max()) <= 1.0 + 1e-3


# ---- 5. isolation -----------------------------------------------------------------------------
def test_precision_switch_leaves_f16x3_untouched():
    """One net rendered in f16x3, then f16, then f16x3: the pack cache is keyed by the precision, so
    the two f16x3 renders are bit-identical and the f16 render differs from them."""
    cfg, arr = fixtures.load("fw_cfg3_nmr")
    net = tgp.hip_net(cfg, arr, "f16x3")
    outs = []
    for prec in ("f16x3", "f16", "f16x3"):
        net.mlp_precision = prec
        r = NeRFRenderer(n_coarse=cfg["n_coarse"], n_fine=cfg["n_fine"], n_fine_depth=cfg["n_fine_depth"],
                         depth_std=cfg["depth_std"], white_bkgd=cfg["white_bkgd"], lindisp=cfg["lindisp"])
        r.streams = (arr["u_coarse"], arr["u_fine"], arr["u_fine_jit"], arr["n_depth"])
        r.return_z = True
        with torch.no_grad():
            outs.append(r(net, arr["rays"].to(DEV), want_weights=True))
    torch.cuda.synchronize()
    a, h, b = outs
    for p in ("coarse", "fine"):
        for k in ("rgb", "depth", "weights", "z"):
            assert torch.equal(a[p][k], b[p][k]), (p, k)
    assert torch.equal(a.coarse.z, h.coarse.z)          # the coarse samples are the streams'
    assert not torch.equal(a.fine.rgb, h.fine.rgb)
    assert not torch.equal(a.coarse.rgb, h.coarse.rgb)


# ---- 6. refusals on the device ----------------------------------------------------------------
def test_grad_paths_refuse_f16_on_device():
    cfg, arr = fixtures.load("fw_cfg3_nmr")
    net = tgp.hip_net(cfg, arr, "f16")
    assert net.needs_grad()
    r = NeRFRenderer(n_coarse=64, n_fine=64, white_bkgd=True)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3'):
            r(net, arr["rays"].to(DEV))
        xyz = torch.zeros(1, 8, 3, device=DEV)
        with pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3'):
            net(xyz, coarse=True, viewdirs=torch.zeros_like(xyz))
    # the gather path has no f16 kernel either
    net.use_latent_proj = False
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r'"f16" is inference only; use f16x3'):
        net(torch.zeros(1, 8, 3, device=DEV), coarse=True, viewdirs=torch.zeros(1, 8, 3, device=DEV))
