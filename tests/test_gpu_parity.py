"""HIP path vs oracle / golden vectors on an MI355X (``-m gpu``).

Tolerance: the fp32 HIP path must match within
    |hip - ref| <= 5e-5 + 1e-5 * |ref|
on rgb / depth / weights / raw model outputs.  The fine pass depends on
searchsorted over the coarse cdf (nerf.py:138), a discontinuous function.  A ray
is excluded from the fine comparison only when a bin flip is PROVEN from the
coarse weights (oracle/parity.py: the bins recomputed from the HIP and the
reference coarse weights with the same u differ); every differing fine sample set
must be such a ray, and at most MAX_FLIPS rays per fixture may flip.
"""
import numpy as np
import pytest
import torch

import fixtures
from oracle import parity, ref_cpu
from pnr import ops, synth
from pnr.models import PixelNeRFNet
from pnr.renderer import NeRFRenderer

pytestmark = pytest.mark.gpu

ATOL, RTOL = 5e-5, 1e-5
MAX_FLIPS = 1          # proven searchsorted flips allowed per fixture (oracle/parity.py)
DEV = "cuda"


def close_mask(a, b, atol=ATOL, rtol=RTOL):
    return (a - b).abs() <= atol + rtol * b.abs()


def assert_close(a, b, what, atol=ATOL, rtol=RTOL):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ok = close_mask(a, b, atol, rtol)
    if not bool(ok.all()):
        d = (a - b).abs()
        i = int(torch.argmax(d.reshape(-1)))
        raise AssertionError("%s: %d/%d outside tol; max |d| %.3g at %d (hip %.7g ref %.7g)" % (
            what, int((~ok).sum()), ok.numel(), float(d.max()), i, float(a.reshape(-1)[i]),
            float(b.reshape(-1)[i])))


def model_conf(n_blocks=5, combine_layer=3):
    mlp = dict(type="resnet", n_blocks=n_blocks, d_hidden=512, combine_layer=combine_layer,
               combine_type="average")
    return dict(use_encoder=True, use_xyz=True, use_code=True,
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True),
                use_viewdirs=True, use_code_viewdirs=False, mlp_coarse=dict(mlp),
                mlp_fine=dict(mlp), encoder=dict(backbone="resnet34", pretrained=False, num_layers=4))


PRECS = ["fp32", "f16x3", "bf16x6", "bf16x9"]


def hip_net(cfg, arr, precision="f16x3", latent_proj=True):
    net = PixelNeRFNet(model_conf(cfg.get("n_blocks", 5), cfg.get("combine_layer", 3)))
    net.mlp_precision = precision
    net.use_latent_proj = latent_proj
    if not cfg.get("with_fine", True):
        net.mlp_fine = None      # as eval_approx.py:62-63 does
    sd = fixtures.state_dict(cfg)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing)
    net = net.to(DEV).eval()
    lat = fixtures.latent_of(cfg).to(DEV)
    sb = cfg.get("sb", 1)
    net.encode_latent(lat, arr["poses"].to(DEV), fixtures.focal_of(arr).to(DEV),
                      (cfg["width"], cfg["height"]),
                      c=None if fixtures.c_or_none(arr) is None else arr["c"].to(DEV), num_objs=sb)
    return net


def hip_render(cfg, arr, want_weights=True, precision="f16x3", latent_proj=True):
    net = hip_net(cfg, arr, precision, latent_proj)
    r = NeRFRenderer(n_coarse=cfg["n_coarse"], n_fine=cfg["n_fine"], n_fine_depth=cfg["n_fine_depth"],
                     depth_std=cfg["depth_std"], white_bkgd=cfg["white_bkgd"], lindisp=cfg["lindisp"])
    r.streams = (arr["u_coarse"], arr["u_fine"], arr["u_fine_jit"], arr["n_depth"])
    r.return_z = True
    with torch.no_grad():
        out = r(net, arr["rays"].to(DEV), want_weights=want_weights)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ kernels --
def test_composite_matches_oracle_random():
    g = torch.Generator().manual_seed(0)
    for B, K, white in [(1, 1, True), (37, 7, False), (300, 64, True), (129, 128, False),
                        (65, 200, True), (65, 300, True)]:
        near, far = 0.3, 4.0
        rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), near),
                          torch.full((B, 1), far)], 1)
        z = torch.sort(near + (far - near) * torch.rand(B, K, generator=g), -1)[0]
        raw = torch.rand(B, K, 4, generator=g)
        raw[..., 3] = torch.randn(B, K, generator=g) * 4.0
        w_ref, rgb_ref, d_ref = ref_cpu.composite(rays, z, raw, white)
        w, rgb, d = ops.composite(z.to(DEV), raw.to(DEV), rays.to(DEV), white)
        assert_close(w, w_ref, "weights B=%d K=%d" % (B, K))
        assert_close(rgb, rgb_ref, "rgb B=%d K=%d" % (B, K))
        assert_close(d, d_ref, "depth B=%d K=%d" % (B, K))


def test_composite_edge_fixture():
    cfg, arr = fixtures.load("composite_edge")
    w, rgb, d = ops.composite(arr["z"].to(DEV), arr["raw"].to(DEV), arr["rays"].to(DEV),
                              cfg["white_bkgd"])
    assert_close(w, arr["weights"], "weights")
    assert_close(rgb, arr["rgb"], "rgb")
    assert_close(d, arr["depth"], "depth")
    assert float(w[:4].abs().max()) == 0.0  # all-zero sigma rays


def test_composite_empty_batch():
    w, rgb, d = ops.composite(torch.zeros(0, 8, device=DEV), torch.zeros(0, 8, 4, device=DEV),
                              torch.zeros(0, 8, device=DEV), True)
    assert rgb.shape == (0, 3) and d.shape == (0,)


def test_composite_unaligned_z_and_weights_through_the_abi():
    """pnr_composite with z and weights at an odd float offset (a view into a larger buffer): z
    and weights are accessed one float at a time, so a misaligned view gives results bit-identical
    to the aligned call; only raw needs 16-B alignment and is refused otherwise."""
    import ctypes

    from pnr import _lib

    def at(t, off=0):
        return ctypes.c_void_p(t.data_ptr() + off)

    g = torch.Generator().manual_seed(5)
    B, K = 67, 128   # K in (64, 128]: the S = 2 kernel
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), 0.3), torch.full((B, 1), 4.0)], 1).to(DEV)
    z = torch.sort(0.3 + 3.7 * torch.rand(B, K, generator=g), -1)[0].to(DEV)
    raw = torch.rand(B, K, 4, generator=g)
    raw[..., 3] = torch.randn(B, K, generator=g) * 4.0
    raw = raw.to(DEV)
    lib = _lib.load()
    st = _lib.stream_of(torch.device(DEV))

    def run(zp, wp):
        rgb = torch.empty(B, 3, device=DEV)
        d = torch.empty(B, device=DEV)
        _lib.check(lib.pnr_composite(zp, at(raw), at(rays), B, K, 1, wp, at(rgb), at(d), st), "pnr_composite")
        return rgb, d

    w0 = torch.empty(B, K, device=DEV)
    rgb0, d0 = run(at(z), at(w0))
    zbuf = torch.empty(B * K + 1, device=DEV)
    zbuf[1:] = z.reshape(-1)
    wbuf = torch.zeros(B * K + 1, device=DEV)
    rgb1, d1 = run(at(zbuf, 4), at(wbuf, 4))
    torch.cuda.synchronize()
    assert torch.equal(rgb0, rgb1) and torch.equal(d0, d1)
    assert torch.equal(w0.reshape(-1), wbuf[1:]) and float(wbuf[0]) == 0.0
    rgb_ref = ref_cpu.composite(rays.cpu(), z.cpu(), raw.cpu(), True)[1]
    assert_close(rgb1, rgb_ref, "rgb (unaligned)")
    rawbuf = torch.empty(B * K * 4 + 1, device=DEV)
    rc = lib.pnr_composite(at(z), at(rawbuf, 4), at(rays), B, K, 1, None, at(rgb0), at(d0), st)
    assert rc != 0


@pytest.mark.parametrize("lindisp", [False, True])
def test_sample_coarse_matches_oracle(lindisp):
    g = torch.Generator().manual_seed(1)
    for B, K in [(5, 1), (64, 32), (1000, 64), (17, 129)]:
        rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), 0.8),
                          torch.full((B, 1), 1.8)], 1)
        u = torch.rand(B, K, generator=g)
        ref = ref_cpu.sample_coarse(rays, K, u, lindisp)
        z = ops.sample_coarse(rays.to(DEV), K, u.to(DEV), lindisp)
        assert_close(z, ref, "z_coarse K=%d" % K, atol=2e-6, rtol=2e-6)


@pytest.mark.parametrize("kc,kf,kfd,lindisp", [(64, 64, 0, False), (64, 32, 16, False),
                                                (16, 12, 4, True), (7, 3, 3, False),
                                                (128, 100, 0, False)])
def test_sample_fine_matches_oracle(kc, kf, kfd, lindisp):
    g = torch.Generator().manual_seed(kc + kf)
    B = 513
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), 0.5),
                      torch.full((B, 1), 3.5)], 1)
    zc = ref_cpu.sample_coarse(rays, kc, torch.rand(B, kc, generator=g), lindisp)
    w = torch.rand(B, kc, generator=g) ** 4
    w[:3] = 0.0                      # all-zero weights -> uniform pdf
    depth = 0.5 + 3.0 * torch.rand(B, generator=g)
    nf = kf - kfd
    u = torch.rand(B, nf, generator=g)
    if nf > 0:
        u[:4, 0] = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))  # u >= cdf[-1]
    uj = torch.rand(B, nf, generator=g)
    nd = torch.randn(B, kfd, generator=g)
    samps = [zc]
    if nf > 0:
        samps.append(ref_cpu.sample_fine(rays, w, kc, u, uj, lindisp))
    if kfd > 0:
        samps.append(ref_cpu.sample_fine_depth(rays, depth, kfd, 0.01, nd))
    ref = torch.sort(torch.cat(samps, -1), -1)[0]
    zf = ops.sample_fine(rays.to(DEV), zc.to(DEV), w.to(DEV), depth.to(DEV), kf, kfd, 0.01,
                         u.to(DEV), uj.to(DEV), nd.to(DEV), lindisp).cpu()
    ok = close_mask(zf, ref, 2e-6, 2e-6).all(1)
    # identical weights -> only ulp-level cdf differences can flip a bin
    assert float((~ok).float().mean()) <= 0.002, int((~ok).sum())
    assert_close(zf[ok], ref[ok], "z_fine", 2e-6, 2e-6)


# ------------------------------------------------------------------- model --
def test_latent_project_matches_fp64():
    """pnr_latent_project: lin_z[b].weight . latent at every latent pixel (no bias), the
    per-scene table the kernel blends instead of the per-point lin_z GEMMs, vs fp64; SB=2
    objects x NS=3 views, a pixel count that is not a multiple of the 64-row tile."""
    sd = synth.pixelnerf_state(4)
    sb, ns = 2, 3
    lat = synth.latent(9, sb * ns, 512, 7, 9)
    net = PixelNeRFNet(model_conf())
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    poses = synth.srn_poses([10.0 * i for i in range(sb * ns)]).reshape(sb, ns, 4, 4)
    net.encode_latent(lat.to(DEV), poses.to(DEV), torch.tensor(50.0, device=DEV), (64, 64), num_objs=sb)
    for mlp, pre in ((net.mlp_coarse, "mlp_coarse"), (net.mlp_fine, "mlp_fine")):
        proj = mlp.latent_proj(net.code, net.hip_scene(), net.encoder.latent_cl).cpu().reshape(3, -1, 512)
        lat_cl = lat.permute(0, 2, 3, 1).reshape(-1, 512).double()
        for b in range(3):
            w = sd["%s.lin_z.%d.weight" % (pre, b)].double()
            ref = lat_cl @ w.t()
            scale = float((lat_cl.abs() @ w.abs().t()).max())
            err = float((proj[b].double() - ref).abs().max())
            assert err <= 2e-6 * scale, (pre, b, err, scale)
    # cached per (weights, latent); a new latent or a weight update rebuilds it
    p1 = net.mlp_coarse.latent_proj(net.code, net.hip_scene(), net.encoder.latent_cl)
    assert p1 is net.mlp_coarse.latent_proj(net.code, net.hip_scene(), net.encoder.latent_cl)
    with torch.no_grad():
        net.mlp_coarse.lin_z[0].weight.mul_(2.0)
    p2 = net.mlp_coarse.latent_proj(net.code, net.hip_scene(), net.encoder.latent_cl)
    assert p2 is not p1
    torch.testing.assert_close(p2.reshape(3, -1, 512)[0].cpu(), 2.0 * p1.reshape(3, -1, 512)[0].cpu(),
                               rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("latent_proj", [True, False])
@pytest.mark.parametrize("precision", PRECS)
def test_point_query_matches_reference_fixture(precision, latent_proj):
    cfg, arr = fixtures.load("fw_pointquery")
    net = hip_net(dict(cfg, n_blocks=5, combine_layer=3, with_fine=True, d_latent=512,
                       d_hidden=512), arr, precision, latent_proj)
    with torch.no_grad():
        vd = torch.zeros_like(arr["xyz"]).to(DEV)
        oc = net(arr["xyz"].to(DEV), coarse=True, viewdirs=vd)
        of = net(arr["xyz"].to(DEV), coarse=False, viewdirs=vd)
    assert_close(oc, arr["out_coarse"], "point query coarse")
    assert_close(of, arr["out_fine"], "point query fine")


@pytest.mark.parametrize("latent_proj", [True, False])
@pytest.mark.parametrize("precision", PRECS)
def test_point_query_multiview_multiobject_vs_oracle(precision, latent_proj):
    """SB=2 objects x NS=3 views, per-object focal/c; checks the x_sum combine path."""
    torch.manual_seed(0)
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
    net = PixelNeRFNet(model_conf())
    net.mlp_precision = precision
    net.use_latent_proj = latent_proj
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    net.encode_latent(lat.to(DEV), poses.to(DEV), focal.to(DEV), (64, 60), c=c.to(DEV), num_objs=sb)
    with torch.no_grad():
        out = net(xyz.to(DEV), coarse=True, viewdirs=vd.to(DEV))
    assert_close(out, ref, "point query SB=2 NS=3")


@pytest.mark.parametrize("latent_proj", [True, False])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("lat_scale,w_scale", [(1e-4, 1.0), (1e3, 1.0), (1.0, 1e-3), (0.0, 1.0)])
def test_point_query_dynamic_range(precision, lat_scale, w_scale, latent_proj):
    """Scaled-fp16 mode keeps fp32-level error when the latent / lin_z weights are far
    from unit scale (per-column and per-layer power-of-two scaling), and on all-zero
    latent columns.  Tolerance relative to the output's magnitude."""
    sd = synth.pixelnerf_state(5)
    for k in list(sd):
        if ".lin_z." in k and k.endswith("weight"):
            sd[k] = sd[k] * w_scale
    lat = synth.latent(11, 1, 512, 16, 16) * lat_scale
    poses = synth.srn_poses([10.0])
    focal = torch.tensor(40.0)
    xyz = torch.from_numpy(synth.hash_sym(91, (1, 300, 3), 0.5))
    vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(92, (1, 300, 3), 1.0)), dim=-1)
    scene = ref_cpu.Scene(lat, poses, focal, 64, 64, None)
    with torch.no_grad():
        ref = ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd)
    net = PixelNeRFNet(model_conf())
    net.mlp_precision = precision
    net.use_latent_proj = latent_proj
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    net.encode_latent(lat.to(DEV), poses.to(DEV), focal.to(DEV), (64, 64))
    with torch.no_grad():
        out = net(xyz.to(DEV), coarse=True, viewdirs=vd.to(DEV)).cpu()
    mag = float(ref.abs().max())
    assert torch.isfinite(out).all()
    assert_close(out, ref, "dynamic range lat*%g w*%g" % (lat_scale, w_scale),
                 atol=ATOL * max(1.0, mag))


@pytest.mark.parametrize("latent_proj", [True, False])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_point_query_nan_point_stays_confined(precision, latent_proj):
    """the f16x3 column maxima use NaN-propagating v_maximum3, so a NaN activation
    makes its column's maximum NaN and that column is split unscaled.  A column of the LDS image is
    ONE point (rows are channels), and a NaN channel reaches every channel of its point at the next
    GEMM, as in torch, so the point is NaN either way; no other point of its tile is affected.
    Checked: NaN view directions on 3 points of 3 different tiles; those points are NaN in the HIP
    output and in the oracle, every other point matches the oracle within the tolerance."""
    sd = synth.pixelnerf_state(5)
    lat = synth.latent(11, 1, 512, 16, 16)
    poses = synth.srn_poses([10.0])
    focal = torch.tensor(40.0)
    xyz = torch.from_numpy(synth.hash_sym(91, (1, 300, 3), 0.5))
    vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(92, (1, 300, 3), 1.0)), dim=-1)
    bad = [5, 70, 200]
    vd[0, bad] = float("nan")
    scene = ref_cpu.Scene(lat, poses, focal, 64, 64, None)
    with torch.no_grad():
        ref = ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd)
    net = PixelNeRFNet(model_conf())
    net.mlp_precision = precision
    net.use_latent_proj = latent_proj
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    net.encode_latent(lat.to(DEV), poses.to(DEV), focal.to(DEV), (64, 64))
    with torch.no_grad():
        out = net(xyz.to(DEV), coarse=True, viewdirs=vd.to(DEV)).cpu()
    good = torch.ones(300, dtype=torch.bool)
    good[bad] = False
    assert bool(torch.isnan(ref[0, bad]).all()) and bool(torch.isnan(out[0, bad]).all())
    assert_close(out[0, good], ref[0, good], "points beside NaN points")


def heavy_tailed_state(seed):
    """Trained-like weight statistics for the accuracy check of the split arithmetics: every
    ResnetFC matrix gets log-normal row and column scales (exp(1.5 N), a ~e^+-4.5 spread per
    side) and 0.2 % outlier entries x 30, then is renormalised to its original Frobenius norm
    so activations stay O(1); the latent gets log-normal per-channel scales (exp(2 N))."""
    sd = synth.pixelnerf_state(seed)
    g = torch.Generator().manual_seed(seed)
    for k in sorted(sd):
        v = sd[k]
        if not k.endswith("weight") or v.dim() != 2 or not k.startswith("mlp_"):
            continue
        r = torch.exp(1.5 * torch.randn(v.shape[0], 1, generator=g))
        c = torch.exp(1.5 * torch.randn(1, v.shape[1], generator=g))
        w = v * r * c
        out = torch.rand(v.shape, generator=g) < 0.002
        w = torch.where(out, w * 30.0, w)
        sd[k] = (w * (v.norm() / w.norm().clamp_min(1e-30))).contiguous()
    return sd


@pytest.mark.parametrize("latent_proj", [True, False])
@pytest.mark.parametrize("precision", PRECS)
def test_point_query_heavy_tailed_weights(precision, latent_proj):
    """the split arithmetics (f16x3: per-layer weight scale, per-column
    image scales; bf16x6 / x9) on heavy-tailed, trained-like weights and latent channels
    (heavy_tailed_state) against the fp32 oracle, tolerance relative to the output magnitude
    as in test_point_query_dynamic_range."""
    sd = heavy_tailed_state(21)
    ch = torch.exp(2.0 * torch.randn(512, generator=torch.Generator().manual_seed(3)))
    lat = synth.latent(12, 1, 512, 16, 16) * ch[None, :, None, None]
    poses = synth.srn_poses([10.0])
    focal = torch.tensor(40.0)
    xyz = torch.from_numpy(synth.hash_sym(93, (1, 512, 3), 0.5))
    vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(94, (1, 512, 3), 1.0)), dim=-1)
    scene = ref_cpu.Scene(lat, poses, focal, 64, 64, None)
    with torch.no_grad():
        ref = ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd)
    net = PixelNeRFNet(model_conf())
    net.mlp_precision = precision
    net.use_latent_proj = latent_proj
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    net.encode_latent(lat.to(DEV), poses.to(DEV), focal.to(DEV), (64, 64))
    with torch.no_grad():
        out = net(xyz.to(DEV), coarse=True, viewdirs=vd.to(DEV)).cpu()
    mag = float(ref.abs().max())
    assert torch.isfinite(out).all() and float(ref[..., 3].abs().max()) > 0   # sigma not all clipped
    assert_close(out, ref, "heavy-tailed weights", atol=ATOL * max(1.0, mag))


@pytest.mark.parametrize("latent_proj", [True, False])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_point_query_camera_plane_and_behind_camera(precision, latent_proj):
    """SURVEY §8(a) a11 edge cases against the oracle's grid_sample border semantics
    (encoder.py:102-108): points ON the source camera plane (x_cam.z == 0 exactly, so
    uv = -x/0 = +-inf, or NaN when x_cam.xy == 0 too: +inf -> W_l - 1, -inf -> 0,
    NaN -> 0 after the border clamp), and points BEHIND the camera (x_cam.z > 0: mirrored
    uv, not masked).  The camera is axis-aligned at z = 1.3 so x_cam.z = x.z - 1.3 is
    exactly 0 in fp32 for x.z = 1.3."""
    sd = synth.pixelnerf_state(8)
    lat = synth.latent(12, 1, 512, 16, 20)
    pose = torch.eye(4)
    pose[2, 3] = 1.3
    P = 256
    g = torch.Generator().manual_seed(4)
    xyz = torch.rand(1, P, 3, generator=g) * 2.0 - 1.0
    xyz[0, :64, 2] = 1.3                 # on the camera plane: +-inf uv
    xyz[0, :4, :2] = 0.0                 # on the camera centre: 0 / 0 = NaN uv
    xyz[0, 4:8, 0] = 0.0                 # x = 0: NaN u, +-inf v
    xyz[0, 64:128, 2] = 1.3 + torch.rand(64, generator=g) * 2.0   # behind the camera
    vd = torch.nn.functional.normalize(torch.randn(1, P, 3, generator=g), dim=-1)
    scene = ref_cpu.Scene(lat, pose[None], torch.tensor(30.0), 80, 64, None)
    with torch.no_grad():
        ref = ref_cpu.pixelnerf_forward(sd, scene, xyz, True, vd)
    assert torch.isfinite(ref).all()
    net = PixelNeRFNet(model_conf())
    net.mlp_precision = precision
    net.use_latent_proj = latent_proj
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    net.encode_latent(lat.to(DEV), pose[None].to(DEV), torch.tensor(30.0, device=DEV), (80, 64))
    with torch.no_grad():
        out = net(xyz.to(DEV), coarse=True, viewdirs=vd.to(DEV)).cpu()
    assert_close(out[0, :64], ref[0, :64], "camera plane (inf / NaN uv)")
    assert_close(out[0, 64:128], ref[0, 64:128], "behind the camera")
    assert_close(out, ref, "all points")


# ------------------------------------------------------------------- rays --
def test_gen_rays_matches_reference_fixture():
    """pnr_gen_rays (util.gen_rays on device poses) vs the reference's util.gen_rays
    (tests/golden/gen_rays.npz): fx/fy + principal point, and scalar focal with the default
    image-centre principal point; 3x4 poses too."""
    from pnr import util

    cfg, arr = fixtures.load("gen_rays")
    poses = arr["poses"].to(DEV)
    r1 = util.gen_rays(poses, cfg["w1"], cfg["h1"], arr["focal1"].to(DEV), cfg["near1"], cfg["far1"],
                       c=arr["c1"].to(DEV))
    r2 = util.gen_rays(poses[:2], cfg["w2"], cfg["h2"], torch.tensor(cfg["focal2"]), cfg["near2"],
                       cfg["far2"])
    r3 = util.gen_rays(poses[:, :3].contiguous(), cfg["w1"], cfg["h1"], arr["focal1"], cfg["near1"],
                       cfg["far1"], c=arr["c1"])
    assert r1.is_cuda and r2.is_cuda
    assert_close(r1, arr["rays1"], "gen_rays focal (2,) + c", atol=2e-6, rtol=0)
    assert_close(r2, arr["rays2"], "gen_rays scalar focal", atol=2e-6, rtol=0)
    assert_close(r3, arr["rays1"], "gen_rays 3x4 poses", atol=2e-6, rtol=0)


# ------------------------------------------------------------------ render --
def fixture_oracle(cfg, arr):
    """(sd, scene, model_kw, white_bkgd, rays_per_obj) of a golden fixture, for the oracle fine
    pass at a flipped ray's own samples (parity.check_flipped_outputs)."""
    sd = fixtures.state_dict(cfg)
    scene = ref_cpu.Scene(fixtures.latent_of(cfg), arr["poses"], fixtures.focal_of(arr), cfg["width"],
                          cfg["height"], fixtures.c_or_none(arr))
    kw = dict(d_latent=cfg["d_latent"], n_blocks=cfg.get("n_blocks", 5),
              combine_layer=cfg.get("combine_layer", 3), has_fine=cfg.get("with_fine", True))
    B = arr["rays"].reshape(-1, 8).shape[0]
    return sd, scene, kw, bool(cfg["white_bkgd"]), B // cfg.get("sb", 1)


def check_flips(name, out, rays, flip_idx, oracle, u_fine=None):
    """Every flipped fine ray's HIP rgb / depth / weights against the oracle fine pass at the
    HIP's own fine samples (nerf.py:284-301 at z_fine_hip): no ray escapes an output check."""
    if not flip_idx:
        return None
    assert oracle is not None, "%s: flipped rays %s and no oracle to check their outputs" % (name, flip_idx)
    sd, scene, kw, white, rpo = oracle
    f = out.fine
    res = parity.check_flipped_outputs(sd, scene, rays, f.z, f.rgb, f.depth, f.weights, flip_idx, rpo, white,
                                       kw, w_coarse_hip=out.coarse.weights, u_fine=u_fine)
    print("%s: flipped rays %s, boundary distance %s, max |d| vs the oracle fine pass at their own "
          "samples %s" % (name, flip_idx, res.get("boundary_distance"), res["max_abs"]))
    assert res["ok"], "%s: flipped rays %s do not match the oracle fine pass at their own samples: %s" % (
        name, res["bad_rays"], res)
    return res


def compare_render(name, out, cfg, arr, max_flips=MAX_FLIPS, oracle=None):
    """Coarse pass at full tolerance.  Fine pass classified by cause (oracle/parity.py): a
    ray is excluded only when the importance-sample bins recomputed from the HIP and the
    reference coarse weights differ (a proven searchsorted flip), and its HIP fine samples
    must then be exactly the reference algorithm's draw from the HIP coarse outputs; every
    returned fine sample set that differs must be such a ray, all other rays are held to
    the full tolerance on rgb / depth / weights / z, and at most ``max_flips`` rays may flip
    besides the fixture's ``force_u_high`` rays (u = 1 - 2^-24 >= cdf[-1] by construction:
    draws placed ON the last cdf boundary)."""
    c = out.coarse
    assert_close(c.rgb, arr["coarse_rgb"], name + " coarse rgb")
    assert_close(c.depth, arr["coarse_depth"], name + " coarse depth")
    assert_close(c.weights, arr["coarse_weights"], name + " coarse weights")
    if "z" in c and "z_coarse" in arr:
        assert_close(c.z.reshape(arr["z_coarse"].shape), arr["z_coarse"], name + " z_coarse", atol=2e-6, rtol=2e-6)
    if cfg["n_fine"] == 0:
        assert "fine" not in out
        return 0
    f = out.fine
    B = arr["fine_rgb"].reshape(-1, 3).shape[0]
    rgb = f.rgb.reshape(B, 3).cpu()
    depth = f.depth.reshape(B).cpu()
    w = f.weights.reshape(B, -1).cpu()
    assert "z" in f and "z" in c, "render with renderer.return_z = True"
    streams = (arr["u_coarse"], arr["u_fine"], arr["u_fine_jit"], arr["n_depth"])
    z_exp = parity.expected_fine_sets(arr["rays"], c.z, c.weights, c.depth, streams, c.z.shape[-1],
                                   cfg["n_fine"], cfg.get("n_fine_depth", 0), cfg.get("depth_std", 0.01),
                                   cfg.get("lindisp", False))
    cls = parity.classify_fine(c.weights.reshape(B, -1), arr["coarse_weights"].reshape(B, -1),
                               arr["u_fine"].reshape(B, -1), f.z.reshape(B, -1), arr["z_fine"].reshape(B, -1),
                               z_exp)
    unexplained = torch.nonzero(cls["unexplained"]).reshape(-1).tolist()
    assert not unexplained, "%s: fine samples differ on rays %s with no searchsorted bin flip" % (
        name, unexplained)
    bad = torch.nonzero(cls["inconsistent"]).reshape(-1).tolist()
    assert not bad, "%s: flipped rays %s do not follow their own coarse weights" % (name, bad)
    forced = set(range(cfg.get("force_u_high", 0)))
    free = [i for i in cls["flip_idx"] if i not in forced]
    assert len(free) <= max_flips, "%s: %d rays flipped fine bins: %s" % (name, len(free), free)
    keep = ~cls["flip"]
    assert_close(f.z.reshape(B, -1).cpu()[keep], arr["z_fine"].reshape(B, -1)[keep], name + " z_fine")
    assert_close(rgb[keep], arr["fine_rgb"].reshape(B, 3)[keep], name + " fine rgb")
    assert_close(depth[keep], arr["fine_depth"].reshape(B)[keep], name + " fine depth")
    assert_close(w[keep], arr["fine_weights"].reshape(B, -1)[keep], name + " fine weights")
    if cls["flip_idx"]:
        if oracle is None and "seed" in cfg:
            oracle = fixture_oracle(cfg, arr)
        check_flips(name, out, arr["rays"], cls["flip_idx"], oracle, arr["u_fine"])
    return len(cls["flip_idx"])


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", ["fw_cfg2", "fw_shipped", "fw_cfg1", "fw_dtu_ns3", "fw_cfg3_nmr",
                                  "fw_cfg2_b128"])
def test_render_matches_reference_fixture(name, precision):
    cfg, arr = fixtures.load(name)
    out = hip_render(cfg, arr, precision=precision)
    n = compare_render(name, out, cfg, arr)
    print("%s/%s: proven fine-bin flips %d" % (name, precision, n))


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["fw_cfg2", "fw_shipped", "fw_dtu_ns3", "fw_cfg3_nmr"])
def test_render_gather_path_matches_reference_fixture(name, precision):
    """The per-point lin_z GEMM path (use_latent_proj = False: latent gather + lin_z on the
    MFMA chain, the training forward's arithmetic) against the same fixtures."""
    cfg, arr = fixtures.load(name)
    out = hip_render(cfg, arr, precision=precision, latent_proj=False)
    compare_render(name + "/gather", out, cfg, arr)


def test_render_multiobject_vs_oracle():
    """SB=2 objects, NS=2 views, shipped 64/32/16 sampling, via bind_parallel."""
    sb, ns, bp = 2, 2, 24
    sd = synth.pixelnerf_state(6)
    lat = synth.latent(10, sb * ns, 512, 20, 24)
    poses = synth.srn_poses([0.0, 40.0, 90.0, 130.0], radius=1.4).reshape(sb, ns, 4, 4)
    focal = torch.tensor(90.0)
    tgt = synth.srn_poses([20.0, 110.0], radius=1.4)
    from pnr import util

    rays = util.gen_rays(tgt, 96, 80, focal, 0.4, 2.4).reshape(sb, -1, 8)
    idx = torch.from_numpy((synth.hash_uniform(3, bp) * rays.shape[1]).astype("int64"))
    rays = rays[:, idx].contiguous()
    streams = synth.rng_streams(5, sb * bp, 64, 32, 16)
    scene = ref_cpu.Scene(lat, poses, focal, 96, 80, None)

    def model_fn(pts, coarse, dirs):
        return ref_cpu.pixelnerf_forward(sd, scene, pts, coarse, dirs)

    with torch.no_grad():
        ref = ref_cpu.render(model_fn, rays, 64, 32, 16, streams, True)
    net = PixelNeRFNet(model_conf())
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    net.encode_latent(lat.to(DEV), poses.to(DEV), focal.to(DEV), (96, 80), num_objs=sb)
    r = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True)
    r.streams = streams
    r.return_z = True
    par = r.bind_parallel(net, [0], simple_output=False)
    with torch.no_grad():
        out = par(rays.to(DEV), want_weights=True)
    arr = dict(coarse_rgb=ref["coarse"]["rgb"], coarse_depth=ref["coarse"]["depth"],
               coarse_weights=ref["coarse"]["weights"], fine_rgb=ref["fine"]["rgb"],
               fine_depth=ref["fine"]["depth"], fine_weights=ref["fine"]["weights"],
               z_fine=ref["fine"]["z"], z_coarse=ref["coarse"]["z"], rays=rays, u_coarse=streams[0],
               u_fine=streams[1], u_fine_jit=streams[2], n_depth=streams[3])
    from pnr.renderer import DotMap

    out = DotMap(coarse=DotMap(out["coarse"]), fine=DotMap(out["fine"]))
    compare_render("multiobject", out, dict(n_fine=32, n_fine_depth=16), arr,
                   oracle=(sd, scene, {}, True, bp))


def test_simple_output_and_empty_rays():
    cfg, arr = fixtures.load("fw_cfg1")
    net = hip_net(cfg, arr)
    r = NeRFRenderer(n_coarse=32, n_fine=0, white_bkgd=True)
    par = r.bind_parallel(net, [0], simple_output=True)
    with torch.no_grad():
        rgb, depth = par(torch.zeros(0, 8, device=DEV))
        assert rgb.shape == (0, 3) and depth.shape == (0,)
        r.streams = (arr["u_coarse"], arr["u_fine"], arr["u_fine_jit"], arr["n_depth"])
        rgb, depth = par(arr["rays"].to(DEV))
    assert_close(rgb, arr["coarse_rgb"], "simple rgb")
    assert_close(depth, arr["coarse_depth"], "simple depth")


def test_render_large_batch_properties():
    """cfg2 at full size (4096 rays x (64 + 64)): size-independent invariants."""
    sd = synth.pixelnerf_state(1)
    sc = synth.scene_srn(seed=0, n_rays=4096, pick="all")
    net = PixelNeRFNet(model_conf())
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    net.encode_latent(sc["latent"].to(DEV), sc["poses"].to(DEV), sc["focal"].to(DEV), (128, 128))
    r = NeRFRenderer(n_coarse=64, n_fine=64, white_bkgd=True)
    torch.manual_seed(3)
    rays = sc["rays"].to(DEV)[None]
    with torch.no_grad():
        out = r(net, rays, want_weights=True)
        # determinism: same streams -> bitwise identical result
        torch.manual_seed(3)
        out2 = r(net, rays, want_weights=True)
    for p in ("coarse", "fine"):
        w = out[p].weights
        assert torch.equal(out[p].rgb, out2[p].rgb) and torch.equal(w, out2[p].weights)
        assert bool((w >= 0).all()) and float(w.sum(-1).max()) <= 1.0 + 1e-5
        assert bool(torch.isfinite(out[p].rgb).all())
        assert float(out[p].rgb.min()) >= -1e-6 and float(out[p].rgb.max()) <= 1.0 + 1e-5
    # the fine pass composite equals a standalone composite of its own samples
    B = 4096
    assert out.fine.weights.shape == (1, B, 128)


def test_render_repeatable_under_memory_contention():
    """The shipped lin_z stage (stage_proj_runs: run-deduplicated corner-row loads blended into
    the LDS stage) under slow loads: the round-3 stagger's nondeterminism appeared only while the
    stage's loads competed with a weight stream ("The round-3 stagger's
    nondeterminism").  Here the cfg2 render (4096 rays x (64 + 64), projected latent) runs once
    alone and twice while a side stream streams 2 x 1 GiB copies through HBM / L2 beside it (the
    copy's workgroups take CUs first, k_point_mlp's persistent workgroups fill the rest and load
    under that traffic); all three are bitwise identical."""
    sd = synth.pixelnerf_state(1)
    sc = synth.scene_srn(seed=0, n_rays=4096, pick="all")
    net = PixelNeRFNet(model_conf())
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    assert net.use_latent_proj
    net.encode_latent(sc["latent"].to(DEV), sc["poses"].to(DEV), sc["focal"].to(DEV), (128, 128))
    r = NeRFRenderer(n_coarse=64, n_fine=64, white_bkgd=True)
    rays = sc["rays"].to(DEV)[None]
    src = torch.empty(1 << 28, device=DEV)
    dst = torch.empty_like(src)
    side = torch.cuda.Stream()
    outs = []
    with torch.no_grad():
        for noisy in (False, True, True):
            torch.manual_seed(5)
            torch.cuda.synchronize()
            if noisy:
                with torch.cuda.stream(side):
                    for _ in range(2):
                        dst.copy_(src)
            out = r(net, rays, want_weights=True)
            outs.append({p: (out[p].rgb.clone(), out[p].depth.clone(), out[p].weights.clone())
                         for p in ("coarse", "fine")})
            torch.cuda.synchronize()
    for o in outs[1:]:
        for p in ("coarse", "fine"):
            for a, b in zip(outs[0][p], o[p]):
                assert torch.equal(a, b), p


def test_full_frame_dtu_ns3_properties_and_fixture_rows():
    """cfg4 at full size: one 400x300 frame (120,000 rays) with NS = 3 source views and the
    real 150x200 latent per view (the multi-view mean path).  The fixture fw_dtu_ns3 holds
    64 hashed pixels of this very frame (synth.scene_multiview(seed=8)); the full-frame
    render gets the fixture's random streams at those rows, so those 64 rays are checked
    against the REFERENCE inside the 120k-ray launch.  All rays: weights >= 0, sum <= 1,
    finite rgb in [0, 1] (black background), and a second render is bitwise identical."""
    import numpy as np
    from pnr import util

    cfg, arr = fixtures.load("fw_dtu_ns3")
    net = hip_net(cfg, arr)
    sc = synth.scene_multiview(seed=8, n_views=3, n_rays=1)
    tgt = synth.srn_poses([10.0], phi=-12.0, radius=2.0)
    rays = util.gen_rays(tgt, 400, 300, sc["focal"], 0.1, 5.0, c=sc["c"]).reshape(-1, 8)
    B = rays.shape[0]
    idx = torch.from_numpy((synth.hash_uniform(8 + 23, 64) * B).astype(np.int64))
    assert torch.equal(rays[idx], arr["rays"].reshape(-1, 8))
    assert len(set(idx.tolist())) == 64
    streams = list(synth.rng_streams(77, B, 64, 64, 0))
    for i, k in enumerate(("u_coarse", "u_fine", "u_fine_jit", "n_depth")):
        if streams[i].shape[1]:
            streams[i][idx] = arr[k]
    outs = []
    for _ in range(2):
        r = NeRFRenderer(n_coarse=64, n_fine=64, white_bkgd=False)
        r.streams = tuple(streams)
        r.return_z = True
        with torch.no_grad():
            outs.append(r(net, rays[None].to(DEV), want_weights=True))
    torch.cuda.synchronize()
    out = outs[0]
    for p in ("coarse", "fine"):
        w = out[p].weights
        assert torch.equal(out[p].rgb, outs[1][p].rgb) and torch.equal(w, outs[1][p].weights)
        assert bool((w >= 0).all()) and float(w.sum(-1).max()) <= 1.0 + 1e-5
        assert bool(torch.isfinite(out[p].rgb).all())
        assert float(out[p].rgb.min()) >= -1e-6 and float(out[p].rgb.max()) <= 1.0 + 1e-5
    from pnr.renderer import DotMap

    rows = idx.to(DEV)
    sub = DotMap({p: DotMap({k: v[:, rows] for k, v in out[p].items()}) for p in ("coarse", "fine")})
    n = compare_render("cfg4 full frame, fixture rows", sub, cfg, arr)
    print("cfg4 full frame: proven fine-bin flips on the fixture rows: %d" % n)


def test_unsupported_config_takes_callback_path_and_misuse_fails_loudly():
    """A conf the fused kernel does not implement (here d_hidden = 256 for the coarse MLP)
    renders through the callback path (tests/test_gpu_fallback.py pins it to the reference);
    the fused path still refuses a model that was never encoded and CPU rays."""
    conf = model_conf()
    conf["mlp_coarse"] = dict(conf["mlp_coarse"], d_hidden=256)
    net = PixelNeRFNet(conf).to(DEV).eval()
    assert "512" in net.fused_conf_reason()
    net.encode_latent(torch.zeros(1, 512, 8, 8, device=DEV), synth.srn_poses([0.0]).to(DEV),
                      torch.tensor(100.0, device=DEV), (64, 64))
    with torch.no_grad():
        out = net(torch.zeros(1, 4, 3, device=DEV), coarse=True, viewdirs=torch.zeros(1, 4, 3, device=DEV))
    assert out.shape == (1, 4, 4) and bool(torch.isfinite(out).all())
    fused = PixelNeRFNet(model_conf()).to(DEV).eval()
    assert fused.fused_conf_reason() is None
    with torch.no_grad(), pytest.raises(NotImplementedError, match="encode"):
        fused(torch.zeros(1, 4, 3, device=DEV), coarse=True, viewdirs=torch.zeros(1, 4, 3, device=DEV))
    with torch.no_grad(), pytest.raises(ValueError, match="HIP device"):
        NeRFRenderer(n_coarse=8)(net, torch.zeros(1, 4, 8))


# ------------------------------------------------------------- video frame --
def test_frame_render_matches_reference_gen_video():
    """gen_video.py:174-236 counterpart (pnr.video): one 32x32 frame through
    render_par = bind_parallel(net, simple_output=True), shipped conf (64 + 32 incl. 16
    depth), vs the reference's frame.  Pixels are excluded only for a proven bin flip
    (the fixture holds the reference's coarse weights and fine samples; the same frame is
    rendered once more with weights and z to classify it); uint8 frames equal except where
    rgb * 255 sits within the fp32 tolerance of an integer (truncation boundary)."""
    from pnr import video

    cfg, arr = fixtures.load("frame32")
    net = PixelNeRFNet(model_conf())
    net.load_state_dict(synth.pixelnerf_state(cfg["seed"]), strict=False)
    net = net.to(DEV).eval()
    lat = synth.latent(cfg["latent_seed"], 1, 512, 64, 64)
    net.encode_latent(lat.to(DEV), arr["poses"].to(DEV), arr["focal"].to(DEV), (cfg["width"], cfg["height"]))
    streams = (arr["u_coarse"], arr["u_fine"], arr["u_fine_jit"], arr["n_depth"])
    r = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, depth_std=0.01, white_bkgd=True).to(DEV)
    r.streams = streams
    render_par = r.bind_parallel(net, simple_output=True)
    frames = video.render_frames(render_par, arr["rays"].to(DEV), ray_batch_size=cfg["size"] ** 2).cpu()
    r.streams = streams
    r.return_z = True
    with torch.no_grad():
        full = r(net, arr["rays"].to(DEV).reshape(1, -1, 8), want_weights=True)
    B = cfg["size"] ** 2
    assert torch.equal(full.fine.rgb.reshape(-1, 3).cpu(), frames.reshape(-1, 3))   # same render
    z_exp = parity.expected_fine_sets(arr["rays"], full.coarse.z, full.coarse.weights, full.coarse.depth,
                                      streams, 64, 32, 16)
    cls = parity.classify_fine(full.coarse.weights.reshape(B, -1), arr["coarse_weights"].reshape(B, -1),
                               arr["u_fine"], full.fine.z.reshape(B, -1), arr["z_fine"].reshape(B, -1), z_exp)
    assert not bool(cls["unexplained"].any()), torch.nonzero(cls["unexplained"]).reshape(-1).tolist()
    assert not bool(cls["inconsistent"].any()), torch.nonzero(cls["inconsistent"]).reshape(-1).tolist()
    assert len(cls["flip_idx"]) <= MAX_FLIPS, cls["flip_idx"]
    scene = ref_cpu.Scene(lat, arr["poses"], arr["focal"], cfg["width"], cfg["height"], None)
    check_flips("frame32", full, arr["rays"], cls["flip_idx"],
                (synth.pixelnerf_state(cfg["seed"]), scene, {}, True, B), arr["u_fine"])
    ref = arr["frames"]
    assert frames.shape == ref.shape
    ok = close_mask(frames, ref).reshape(B, 3).all(-1)
    bad = torch.nonzero(~ok & ~cls["flip"]).reshape(-1).tolist()
    assert not bad, "pixels outside tolerance without a bin flip: %s" % bad
    u8 = torch.from_numpy(video.to_uint8(frames)).int().reshape(B, 3)
    ref8 = arr["frames_u8"].int().reshape(B, 3)
    edge = (((ref * 255) - torch.round(ref * 255)).abs() <= 255 * (ATOL + RTOL)).reshape(B, 3)
    diff = (u8 != ref8) & ~cls["flip"][:, None] & ~edge
    assert int(diff.sum()) == 0


# --------------------------------------------------------------- encoder --
@pytest.mark.parametrize("nhwc", [False, True])
def test_latent_channels_last_backward_matches_torch_autograd(nhwc):
    """LatentChannelsLast (the training encoder's upsample + concat, encoder.py:150-160, as one
    HIP kernel) against autograd of F.interpolate(align_corners) + torch.cat + the
    channels-last permute: forward and the gradient of every trunk map, with NCHW maps and with
    channels-last maps (pnr_latent_channels_last_nhwc, the channels-last trunk's)."""
    import torch.nn.functional as F

    from pnr.encoder import LatentChannelsLast

    gen = torch.Generator(device="cpu").manual_seed(5)
    shapes = [(2, 64, 32, 40), (2, 64, 16, 20), (2, 128, 8, 10), (2, 256, 4, 5)]
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    maps = [torch.randn(sh, generator=gen).to(DEV).contiguous(memory_format=fmt).requires_grad_(True)
            for sh in shapes]
    out = LatentChannelsLast.apply(*maps)
    ref = torch.cat([F.interpolate(m, (32, 40), mode="bilinear", align_corners=True) for m in maps],
                    1).permute(0, 2, 3, 1)
    assert (out - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())
    g = torch.randn(out.shape, generator=gen).to(DEV)
    got = torch.autograd.grad(out, maps, g)
    want = torch.autograd.grad(ref, maps, g)
    for a, b in zip(got, want):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item(), (a - b).abs().max().item()


@pytest.mark.parametrize("out_hw,shapes", [
    ((33, 47), [(3, 8, 33, 47), (3, 16, 17, 24), (3, 32, 9, 12), (3, 64, 5, 6)]),
    ((64, 64), [(4, 64, 64, 64), (4, 64, 32, 32), (4, 128, 16, 16), (4, 256, 8, 8)]),   # cfg5's trunk
    ((7, 9), [(2, 4, 7, 9), (2, 8, 1, 5), (2, 4, 3, 1), (2, 4, 2, 1)]),
])
def test_latent_backward_gather_matches_torch_and_is_deterministic(out_hw, shapes):
    """pnr_latent_channels_last_backward (the adjoint gather for channels-last maps) against
    torch's upsample_bilinear2d_backward on odd scales, 1-pixel maps and cfg5's trunk sizes;
    bitwise repeatable (torch's scatter is atomic)."""
    import torch.nn.functional as F

    from pnr.encoder import LatentChannelsLast

    gen = torch.Generator(device="cpu").manual_seed(11)
    maps = [torch.randn(sh, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            for sh in shapes]
    out = LatentChannelsLast.apply(*maps)
    ref = torch.cat([F.interpolate(m, out_hw, mode="bilinear", align_corners=True) for m in maps],
                    1).permute(0, 2, 3, 1)
    g = torch.randn(out.shape, generator=gen).to(DEV)
    got = torch.autograd.grad(out, maps, g, retain_graph=True)
    again = torch.autograd.grad(out, maps, g)
    want = torch.autograd.grad(ref, maps, g)
    for a, b, c in zip(got, want, again):
        assert a.shape == b.shape and a.is_contiguous(memory_format=torch.channels_last)
        assert (a - b).abs().max().item() <= 1e-5 * max(b.abs().max().item(), 1.0), (a - b).abs().max().item()
        assert torch.equal(a, c)


@pytest.mark.parametrize("nhwc", [False, True])
def test_latent_channels_last_matches_torch_upsample_concat(nhwc):
    """pnr_latent_channels_last (encoder.py:150-160 tail; NCHW maps) and
    pnr_latent_channels_last_nhwc (channels-last maps) vs the reference's F.interpolate(bilinear,
    align_corners=True) + cat, transposed; and a no-grad SpatialEncoder.forward on the device
    takes that path (latent_cl written directly)."""
    import torch.nn.functional as F
    from pnr.encoder import SpatialEncoder

    g = torch.Generator().manual_seed(0)
    n = 2
    maps = [torch.randn(n, 64, 48, 56, generator=g), torch.randn(n, 64, 24, 28, generator=g),
            torch.randn(n, 128, 12, 14, generator=g), torch.randn(n, 256, 6, 7, generator=g)]
    ref = torch.cat([F.interpolate(t, (48, 56), mode="bilinear", align_corners=True) for t in maps], 1)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    enc = SpatialEncoder(pretrained=False).to(DEV)
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    with torch.no_grad():
        enc.set_latent_maps([t.to(DEV).contiguous(memory_format=fmt) for t in maps])
    got = enc.latent_cl.cpu()
    assert got.shape == ref.shape
    torch.testing.assert_close(got, ref, atol=1e-5, rtol=0)   # O(1) values: a few ulps
    torch.testing.assert_close(enc.latent.cpu(), ref.permute(0, 3, 1, 2), atol=1e-5, rtol=0)
    # full encoder forward on device under no_grad == the torch path of the same trunk
    img = torch.rand(1, 3, 64, 64, generator=g).to(DEV) * 2 - 1
    enc.eval()
    with torch.no_grad():
        lat_hip = enc(img).clone()
        cl_hip = enc.latent_cl.clone()
    lat_torch = enc(img.requires_grad_(True))   # grad-enabled input: the torch autograd path
    # two separate trunk passes: MIOpen may choose different conv algorithms with / without
    # grad, so the comparison carries the convolutions' own fp32 spread (upsample checked above)
    torch.testing.assert_close(lat_hip, lat_torch.detach(), atol=1e-4, rtol=1e-5)
    torch.testing.assert_close(cl_hip, enc.latent_cl.detach(), atol=1e-4, rtol=1e-5)


def test_eval_encode_inference_trunk_matches_module_path():
    """The eval-mode encode (pnr.encoder.InferenceTrunk: BatchNorm folded into the convolutions,
    trunk + latent kernel replayed as one HIP graph) against the module's own conv / BN / relu
    forward on the same weights, with non-trivial running statistics; a second image replays the
    same graph; an in-place parameter change is picked up; returned latents are not aliased."""
    from pnr.encoder import SpatialEncoder

    g = torch.Generator().manual_seed(3)
    enc = SpatialEncoder(pretrained=False)
    for mod in enc.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            c = mod.num_features
            mod.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.25)
            mod.weight.data.copy_(torch.rand(c, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(c, generator=g) * 0.1)
    enc = enc.to(DEV).eval()
    imgs = [(torch.rand(2, 3, 64, 80, generator=g) * 2 - 1).to(DEV) for _ in range(2)]

    def encode(img, fast):
        enc.infer_fast = fast
        with torch.no_grad():
            enc(img)
        return enc.latent_cl.clone(), enc.latent_cl

    def check(got, want):
        scale = want.abs().max().item()
        d = (got - want).abs().max().item()
        assert d <= 2e-5 * scale, (d, scale)   # fp32 conv spread, relative to the latent's range

    refs = [encode(x, False)[0] for x in imgs]
    first, first_buf = encode(imgs[0], True)
    assert enc._infer is not None and enc._infer.use_graph and len(enc._infer.graphs) == 1
    second, _ = encode(imgs[1], True)            # same shape: the captured graph, new input
    assert len(enc._infer.graphs) == 1
    check(first, refs[0])
    check(second, refs[1])
    assert torch.equal(first_buf, first)         # the first call's latent survived the replay
    again, _ = encode(imgs[0], True)             # a replay of the same input (MIOpen's convolution
    check(again, refs[0])                        # solvers are not all bitwise repeatable)
    with torch.no_grad():
        enc.model.layer2[1].bn2.bias.add_(0.3)   # an in-place update: the fold is refreshed
    ref3 = encode(imgs[0], False)[0]
    got3, _ = encode(imgs[0], True)
    assert not torch.equal(got3, first)
    check(got3, ref3)
    # updates a version-counter key cannot see: through .data, a replaced tensor
    # (load_state_dict(assign=True)), a swapped module; each against the module path
    prev = got3

    def changed():
        nonlocal prev
        ref = encode(imgs[0], False)[0]
        got, _ = encode(imgs[0], True)
        assert not torch.equal(got, prev)
        check(got, ref)
        prev = got

    with torch.no_grad():
        w = enc.model.layer1[1].conv2.weight
        w.data.copy_(w * 1.5)
    changed()
    with torch.no_grad():
        enc.model.layer3[2].bn1.running_var.data.mul_(3.0)
    changed()
    n_graphs = len(enc._infer.graphs)
    sd = {k: (v * 1.1 if k.endswith("bn1.weight") else v).clone() for k, v in enc.state_dict().items()}
    enc.load_state_dict(sd, assign=True)
    changed()
    assert len(enc._infer.graphs) == n_graphs    # same shapes: the graph is kept, the table rewritten
    bn = torch.nn.BatchNorm2d(128, eps=1e-3).to(DEV).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(128, generator=g).to(DEV) * 0.1)
        bn.running_var.copy_((torch.rand(128, generator=g) + 0.5).to(DEV))
    enc.model.layer2[0].bn2 = bn
    changed()
    import copy

    twin = copy.deepcopy(enc)                    # an encoded model copies without its graphs
    assert twin._infer is None
    twin.infer_fast = True
    with torch.no_grad():
        twin(imgs[1])
    check(twin.latent_cl, encode(imgs[1], False)[0])


# ----------------------------------------------------- coarse-output reuse --
@pytest.mark.parametrize("kfd", [0, 16])
def test_fine_pass_reuses_coarse_outputs_when_mlp_fine_is_none(kfd):
    """eval_approx.py --coarse: mlp_fine = None, 64 coarse + 128 fine samples.  The fine pass
    then runs the coarse MLP, so pnr_render_forward_proj evaluates only the new samples and
    merges the coarse pass's outputs.  The result must be BITWISE equal to a render whose fine
    MLP is a separate copy of the coarse one (no reuse), and match the oracle."""
    import copy

    sd = synth.pixelnerf_state(3)
    sc = synth.scene_srn(seed=4, n_rays=96, pick="hash")
    streams = synth.rng_streams(6, 96, 64, 128, kfd)

    def make(share):
        net = PixelNeRFNet(model_conf())
        net.load_state_dict(sd, strict=False)
        if share:
            net.mlp_fine = None
        else:
            net.mlp_fine = copy.deepcopy(net.mlp_coarse)
        net = net.to(DEV).eval()
        net.encode_latent(sc["latent"].to(DEV), sc["poses"].to(DEV), sc["focal"].to(DEV), (128, 128))
        return net

    outs = []
    for share in (True, False):
        r = NeRFRenderer(n_coarse=64, n_fine=128, n_fine_depth=kfd, white_bkgd=True)
        r.streams = streams
        r.return_z = True
        with torch.no_grad():
            outs.append(r(make(share), sc["rays"][None].to(DEV), want_weights=True))
    torch.cuda.synchronize()
    for part in ("coarse", "fine"):
        for k in ("rgb", "depth", "weights"):
            assert torch.equal(outs[0][part][k], outs[1][part][k]), (part, k)
    # oracle: the coarse MLP in both passes
    sd_c = dict(sd)
    for k in list(sd):
        if k.startswith("mlp_fine."):
            sd_c[k] = sd["mlp_coarse." + k[len("mlp_fine."):]]
    scene = ref_cpu.Scene(sc["latent"], sc["poses"], sc["focal"], 128, 128, None)
    with torch.no_grad():
        ref = ref_cpu.render(lambda p, c, d: ref_cpu.pixelnerf_forward(sd_c, scene, p, c, d),
                             sc["rays"][None], 64, 128, kfd, streams, True)
    arr = dict(coarse_rgb=ref["coarse"]["rgb"], coarse_depth=ref["coarse"]["depth"],
               coarse_weights=ref["coarse"]["weights"], fine_rgb=ref["fine"]["rgb"],
               fine_depth=ref["fine"]["depth"], fine_weights=ref["fine"]["weights"], z_fine=ref["fine"]["z"],
               z_coarse=ref["coarse"]["z"], rays=sc["rays"], u_coarse=streams[0], u_fine=streams[1],
               u_fine_jit=streams[2], n_depth=streams[3])
    compare_render("reuse kfd=%d" % kfd, outs[0], dict(n_fine=128, n_fine_depth=kfd), arr,
                   oracle=(sd_c, scene, {}, True, 96))


@pytest.mark.parametrize("name", ["fw_cfg2", "fw_shipped"])
def test_torch_ops_render_rays_matches_fixture(name):
    """torch.ops.pnr.render_rays called directly -- the operator NeRFRenderer.forward dispatches
    to (libpnr_torch.so, TORCH_LIBRARY over pnr_render_forward_proj) -- against the fixture, and
    torch.ops.pnr.composite / point_query against the renderer's own calls."""
    from pnr import torchops
    from pnr.renderer import DotMap

    cfg, arr = fixtures.load(name)
    net = hip_net(cfg, arr)
    ops_ = torchops.load()
    rays = arr["rays"].reshape(-1, 8).to(DEV).contiguous()
    B = rays.shape[0]
    desc, pc = net.hip_mlp(True)
    pf = net.hip_mlp(False)[1]
    st = [arr[k].to(DEV).float().contiguous() for k in ("u_coarse", "u_fine", "u_fine_jit", "n_depth")]
    with torch.no_grad():
        res = ops_.render_rays(*torchops.scene_args(net), torchops.desc_list(desc), pc, pf, net.hip_proj(True),
                               net.hip_proj(False), rays, B // cfg.get("sb", 1), cfg["n_coarse"], cfg["n_fine"],
                               cfg["n_fine_depth"], float(cfg["depth_std"]), bool(cfg["white_bkgd"]),
                               bool(cfg["lindisp"]), *st, 0, 0, True, True)
    torch.cuda.synchronize()
    c_rgb, c_depth, c_w, f_rgb, f_depth, f_w, z_c, z_f = res
    sb = cfg.get("sb", 1)
    out = DotMap(coarse=DotMap(rgb=c_rgb.reshape(sb, -1, 3), depth=c_depth.reshape(sb, -1),
                               weights=c_w.reshape(sb, -1, c_w.shape[-1]), z=z_c.reshape(sb, -1, z_c.shape[-1])),
                 fine=DotMap(rgb=f_rgb.reshape(sb, -1, 3), depth=f_depth.reshape(sb, -1),
                             weights=f_w.reshape(sb, -1, f_w.shape[-1]), z=z_f.reshape(sb, -1, z_f.shape[-1])))
    compare_render(name + "/torch.ops", out, cfg, arr)
    # composite: the operator on the fine samples and the fused march's fine weights agree
    w, rgb, depth = ops_.composite(z_f, torch.rand(B, z_f.shape[-1], 4, device=DEV), rays, True, True)
    assert w.shape == z_f.shape and rgb.shape == (B, 3) and depth.shape == (B,)


# ------------------------------------------------------------- fused ray march --
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("kc,kf,kfd,white,lindisp,n_views,sb", [
    (64, 64, 0, True, False, 1, 1),      # cfg2 / cfg3: both passes fused, fine draws in the coarse epilogue
    (64, 32, 16, True, False, 1, 1),     # shipped conf: coarse fused (+ fine draws), fine pass K = 96 separate
    (64, 0, 0, False, True, 1, 1),       # coarse only
    (128, 0, 0, True, False, 1, 1),      # two tiles per ray
    (32, 32, 0, True, False, 1, 1),      # coarse K = 32 separate, fine K = 64 fused
    (64, 64, 16, False, False, 3, 2),    # multi-view mean, two objects, depth samples
    (64, 64, 16, True, True, 1, 1),      # lindisp + depth samples, per-ray near / far
])
def test_fused_march_matches_unfused(precision, kc, kf, kfd, white, lindisp, n_views, sb):
    """The fused ray march (pnr_render_set_fused: mode 2, the default, sampling + MLP + composite
    in k_point_mlp with the fine draws in their own kernel; mode 1, the fine draws in the coarse
    epilogue too; mode 3, both passes in one launch for the 64 + 64 shapes) is bit-identical to the separate sample / MLP / composite kernels (mode 0) for
    every output, in every arithmetic; the fixture tests above hold the default path to the
    oracle."""
    from pnr import _lib

    from pnr import util

    n_rays = 1024
    sd = synth.pixelnerf_state(1)
    if n_views == 1 and sb == 1:
        sc = synth.scene_srn(seed=5, n_rays=n_rays, pick="all")
        lat, poses, focal, wh, c, rays = sc["latent"], sc["poses"], sc["focal"], (128, 128), None, sc["rays"]
        if lindisp:   # per-ray near / far (the fused epilogue reads them from LDS per ray)
            rays = rays.clone()
            h = torch.from_numpy(synth.hash_uniform(17, n_rays).astype("float32"))
            rays[:, 6] = 0.2 + 0.6 * h
            rays[:, 7] = 2.5 + 1.5 * h
    else:
        lat = synth.latent(10, sb * n_views, 512, 30, 40)
        poses = synth.srn_poses([30.0 * i for i in range(sb * n_views)], radius=1.4).reshape(sb, n_views, 4, 4)
        focal, wh, c = torch.tensor(90.0), (96, 80), None
        rays = util.gen_rays(synth.srn_poses([15.0 + 40.0 * i for i in range(sb)], radius=1.4), 96, 80,
                             focal, 0.4, 2.4).reshape(sb, -1, 8)
        idx = torch.from_numpy((synth.hash_uniform(3, n_rays) * rays.shape[1]).astype("int64"))
        rays = rays[:, idx].contiguous()
    net = PixelNeRFNet(model_conf())
    net.mlp_precision = precision
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    net.encode_latent(lat.to(DEV), poses.to(DEV), focal.to(DEV), wh,
                      c=None if c is None else c.to(DEV), num_objs=sb)
    r = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, depth_std=0.01, white_bkgd=white,
                     lindisp=lindisp)
    r.return_z = True
    rays = rays.to(DEV).reshape(sb, -1, 8)
    outs = []
    # separate kernels, full fusion, fused passes + fine-draw kernel, both passes in one launch
    for mode in (0, 1, 2, 3):
        r.march_mode = mode  # pnr_render_cfg.march_mode (per call, ABI 3)
        with torch.no_grad():
            torch.manual_seed(11)
            outs.append(r(net, rays, want_weights=True))
    # the process default (pnr_render_set_fused) still selects the mode of calls without one
    r.march_mode = None
    with _lib.fused_march(0), torch.no_grad():
        torch.manual_seed(11)
        dflt = r(net, rays, want_weights=True)
    torch.cuda.synchronize()
    for p in (("coarse", "fine") if kf > 0 else ("coarse",)):
        assert torch.equal(dflt[p].rgb, outs[0][p].rgb) and torch.equal(dflt[p].z, outs[0][p].z)
    b = outs[0]
    for mode, a in ((1, outs[1]), (2, outs[2]), (3, outs[3])):
        for p in (("coarse", "fine") if kf > 0 else ("coarse",)):
            for k in ("rgb", "depth", "weights", "z"):
                x, y = getattr(a[p], k, None), getattr(b[p], k, None)
                if y is None:
                    continue
                assert x is not None and torch.equal(x, y), (mode, p, k, float((x - y).abs().max())
                                                             if x is not None else None)
    a = outs[2]
    w = a.coarse.weights
    assert bool((w >= 0).all()) and float(w.sum(-1).max()) <= 1.0 + 1e-5
    # a normal render does not ask for z, and then mode 3's fine tiles read their
    # depths from LDS only (no z_fine in HBM); that path too is bit-identical to mode 0
    r.return_z = False
    for mode in (3, 2):
        r.march_mode = mode
        with torch.no_grad():
            torch.manual_seed(11)
            o = r(net, rays, want_weights=True)
        torch.cuda.synchronize()
        for p in (("coarse", "fine") if kf > 0 else ("coarse",)):
            assert "z" not in o[p]
            for k in ("rgb", "depth", "weights"):
                assert torch.equal(o[p][k], b[p][k]), ("return_z=False", mode, p, k)


@pytest.mark.parametrize("n_views,kc,kf,kfd,streams", [(3, 64, 64, 0, False), (1, 64, 64, 0, True),
                                                       (1, 64, 32, 16, False), (3, 128, 64, 0, False)])
def test_ray_order_is_bit_identical(n_views, kc, kf, kfd, streams):
    """pnr_render_cfg.ray_order (ABI 8, NeRFRenderer.ray_order): the fused march taking the rays in
    16 x 16 pixel blocks gives bit-identical outputs to the input order in march modes 1, 2 and 3,
    with counter-mode draws (keyed by the ray's own index) and injected streams; the raw-output
    path (mlp_fine None: the coarse march writes raw for the fine pass's reuse) too; an order with
    out-of-range entries marches those units' own rays instead of faulting."""
    import ctypes

    from pnr import _lib, torchops, util
    from pnr.renderer import ray_block_order

    W, H = 64, 48
    lat = synth.latent(10, n_views, 512, 30, 40)
    poses = synth.srn_poses([30.0 * i for i in range(n_views)], radius=1.4).reshape(1, n_views, 4, 4)
    focal = torch.tensor(60.0)
    rays = util.gen_rays(synth.srn_poses([15.0], radius=1.4), W, H, focal, 0.4, 2.4).reshape(1, -1, 8).to(DEV)
    order = ray_block_order(rays[0])
    assert order is not None and not torch.equal(order.cpu(), torch.arange(W * H, dtype=torch.int32))
    for fine_none in (False, True):
        net = PixelNeRFNet(model_conf())
        net.load_state_dict(synth.pixelnerf_state(1), strict=False)
        if fine_none:
            net.mlp_fine = None   # as eval_approx.py:62-63 does
        net = net.to(DEV).eval()
        net.encode_latent(lat.to(DEV), poses.to(DEV), focal.to(DEV), (W, H), num_objs=1)
        r = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, depth_std=0.01, white_bkgd=True)
        r.return_z = True
        for mode in ((2,) if fine_none else (1, 2, 3)):
            r.march_mode = mode
            outs = []
            for ro in ("input", "blocked"):
                r.ray_order = ro
                if streams:
                    r.streams = synth.rng_streams(7, W * H, kc, kf, kfd)
                with torch.no_grad():
                    torch.manual_seed(3)
                    outs.append(r(net, rays, want_weights=True))
            torch.cuda.synchronize()
            for p in ("coarse", "fine"):
                for k in ("rgb", "depth", "weights", "z"):
                    x, y = outs[0][p][k], outs[1][p][k]
                    assert torch.equal(x, y), (mode, fine_none, p, k, float((x - y).abs().max()))
    # out-of-range entries: those units march their own index (no fault, same result)
    bad = order.clone()
    bad[:5] = torch.tensor([-1, W * H, 2 ** 30, -7, W * H + 3], dtype=torch.int32, device=DEV)
    bad[5:] = torch.arange(5, W * H, dtype=torch.int32, device=DEV)
    ops_ = torchops.load()
    desc, pc = net.hip_mlp(True)
    res = []
    for ro in (None, bad):
        res.append(ops_.render_rays(*torchops.scene_args(net), torchops.desc_list(desc), pc, pc, net.hip_proj(True),
                                    None, rays[0].contiguous(), W * H, 64, 0, 0, 0.01, True, False, None, None, None,
                                    None, 5, 0, True, False, [], 2, ro))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


def test_march_modes_in_two_host_threads():
    """calls are re-entrant with no mutable globals -- two host threads on one
    device (the DataParallel replicas of nerf.py:370 call from one thread each) render the
    same rays concurrently, one with the separate kernels (march_mode 0) and one with the fused
    march (2), each on its own stream, several times; every result is bit-identical to a
    single-thread render of the fixture rays in mode 2, and the fixture parity holds."""
    import threading

    cfg, arr = fixtures.load("fw_cfg2")
    net = hip_net(cfg, arr)
    rays = arr["rays"].to(DEV)
    st = [arr[k].to(DEV).float() for k in ("u_coarse", "u_fine", "u_fine_jit", "n_depth")]

    def make(mode):
        r = NeRFRenderer(n_coarse=cfg["n_coarse"], n_fine=cfg["n_fine"], n_fine_depth=cfg["n_fine_depth"],
                         depth_std=cfg["depth_std"], white_bkgd=bool(cfg["white_bkgd"]),
                         lindisp=bool(cfg["lindisp"]))
        r.return_z = True
        r.march_mode = mode
        return r

    def render(r):
        r.streams = tuple(st)
        with torch.no_grad():
            return r(net, rays, want_weights=True)

    net.hip_mlp(True), net.hip_mlp(False), net.hip_proj(True), net.hip_proj(False)   # packs built once
    ref = render(make(2))
    compare_render("fw_cfg2/threads-ref", ref, cfg, arr)
    torch.cuda.synchronize()
    results, errors = {}, []

    def worker(mode):
        try:
            s = torch.cuda.Stream(DEV)
            r = make(mode)
            outs = []
            with torch.cuda.stream(s):
                for _ in range(4):
                    outs.append(render(r))
            s.synchronize()
            results[mode] = outs
        except Exception as e:   # surfaced below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(m,)) for m in (0, 2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not errors, errors
    for mode in (0, 2):
        assert len(results[mode]) == 4
        for o in results[mode]:
            for p in ("coarse", "fine"):
                for k in ("rgb", "depth", "weights", "z"):
                    assert torch.equal(o[p][k], ref[p][k]), (mode, p, k)


# ------------------------------------------------------------- bind_parallel --
def test_bind_parallel_replicas_render_fixture():
    """nn.DataParallel (bind_parallel(net, gpus=[...]), nerf.py:354-371; gen_video.py:110,
    train.py:93) re-replicates the network on every forward with torch.nn.parallel.replicate.
    Here two replicas on device 0 (the one-GPU box) are built AFTER the original has packed
    its weights and projected its latent; each renders half of fw_cfg2's rays with the
    fixture's streams for those rays.  Each replica must pack and project from its own
    parameters (the replicas used to inherit the original's packs through their
    __dict__ copy), and the assembled render must match the reference fixture."""
    from torch.nn.parallel import replicate

    from pnr.renderer import DotMap, _RenderWrapper

    cfg, arr = fixtures.load("fw_cfg2")
    net = hip_net(cfg, arr)
    # the reference moves the renderer to the device before bind_parallel (gen_video.py:106-110)
    r = NeRFRenderer(n_coarse=cfg["n_coarse"], n_fine=cfg["n_fine"], n_fine_depth=cfg["n_fine_depth"],
                     depth_std=cfg["depth_std"], white_bkgd=bool(cfg["white_bkgd"]),
                     lindisp=bool(cfg["lindisp"])).to(DEV)
    r.return_z = True
    st = [arr[k].float() for k in ("u_coarse", "u_fine", "u_fine_jit", "n_depth")]
    r.streams = tuple(st)
    with torch.no_grad():
        ref = r(net, arr["rays"].to(DEV), want_weights=True)   # the original packs + projects
    orig_pack = net.mlp_coarse.__dict__["_pnr_pack"].buffers[1]
    wrapped = _RenderWrapper(net, r, simple_output=False)
    reps = replicate(wrapped, [0, 0], detach=True)
    B = arr["rays"].shape[1]
    half = B // 2
    parts = []
    for i, rep in enumerate(reps):
        lo, hi = i * half, (B if i == len(reps) - 1 else (i + 1) * half)
        rep.renderer.streams = tuple(t[lo:hi] for t in st)
        with torch.no_grad():
            o = rep(arr["rays"][:, lo:hi].to(DEV), want_weights=True)
        m = rep.net.mlp_coarse
        own = m.__dict__["_pnr_pack"]
        assert own.owner() is m and own.buffers[1] is not orig_pack, "replica %d reused the original's pack" % i
        assert m.__dict__["_pnr_proj"].owner() is m
        parts.append(o)
    torch.cuda.synchronize()
    out = DotMap({p: DotMap({k: torch.cat([o[p][k] for o in parts], 1) for k in parts[0][p]})
                  for p in ("coarse", "fine")})
    compare_render("fw_cfg2/replicas", out, cfg, arr)
    for p in ("coarse", "fine"):
        for k in ("rgb", "depth", "weights", "z"):
            assert torch.equal(out[p][k], ref[p][k]), (p, k)


def test_bind_parallel_dataparallel_forward():
    """The nn.DataParallel module bind_parallel returns for two device ids (both 0 here):
    every forward re-replicates, each replica renders its scatter chunk of the rays with
    counter-mode draws; the result has the right shapes and the composite invariants, and the
    original's packs are never handed to a replica."""
    cfg, arr = fixtures.load("fw_cfg2")
    net = hip_net(cfg, arr)
    r = NeRFRenderer(n_coarse=64, n_fine=64, white_bkgd=True).to(DEV)
    par = r.bind_parallel(net, [0, 0], simple_output=False)
    rays = arr["rays"].to(DEV)
    with torch.no_grad():
        net.hip_mlp(True), net.hip_proj(True)
        for _ in range(2):
            out = par(rays, want_weights=True)
    torch.cuda.synchronize()
    B = rays.shape[1]
    for p in ("coarse", "fine"):
        assert out[p]["rgb"].shape == (1, B, 3) and out[p]["depth"].shape == (1, B)
        w = out[p]["weights"]
        assert bool((w >= 0).all()) and float(w.sum(-1).max()) <= 1.0 + 1e-5
        assert bool(torch.isfinite(out[p]["rgb"]).all())


def test_single_launch_uses_each_pack_pe_table():
    """march mode 3 runs the coarse and the fine tiles in one launch; the fine
    tiles must read the positional-encoding table from the FINE pack's header.  Here the two packs
    carry different tables (the fine MLP packed with another freq_factor, as two separately built
    models could); mode 3 must stay bit-identical to mode 0, whose separate launches each read
    their own pack."""
    from pnr import torchops
    from pnr.models import PositionalEncoding

    cfg, arr = fixtures.load("fw_cfg2")
    net = hip_net(cfg, arr)
    ops_ = torchops.load()
    rays = arr["rays"].reshape(-1, 8).to(DEV).contiguous()
    B = rays.shape[0]
    desc, pc = net.hip_mlp(True)
    code2 = PositionalEncoding(6, 3, 2.5, True).to(DEV)
    _, pf = net.mlp_fine.packed(code2, net.mlp_precision)
    zc, zf = net.hip_proj(True), net.hip_proj(False)
    outs = {}
    for mode in (0, 3):
        with torch.no_grad():
            outs[mode] = ops_.render_rays(*torchops.scene_args(net), torchops.desc_list(desc), pc, pf, zc, zf, rays,
                                          B, 64, 64, 0, 0.01, True, False, None, None, None, None, 1234, 0, True,
                                          True, [], mode)
    torch.cuda.synchronize()
    for a, b in zip(outs[0], outs[3]):
        assert torch.equal(a, b)
    # and the tables really differ: the fine pass with the coarse table is another render
    with torch.no_grad():
        other = ops_.render_rays(*torchops.scene_args(net), torchops.desc_list(desc), pc, net.hip_mlp(False)[1], zc,
                                 zf, rays, B, 64, 64, 0, 0.01, True, False, None, None, None, None, 1234, 0, True,
                                 True, [], 0)
    assert not torch.equal(other[3], outs[0][3])


# ----------------------------------------------------- encoder vs the reference --
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("fast", [False, True])
def test_encode_matches_reference_encoder_fixture(fast, layout):
    """PixelNeRFNet.encode's latent against the REFERENCE's SpatialEncoder.forward (encoder.py:111-164,
    tests/golden/encoder_fw.npz made by tests/golden/make_encoder_golden.py on the same hashed
    weights): every eval case (use_first_pool, num_layers 3 / 4, feature_scale 1 / 0.5) through the
    module path (fast False) and the BN-folded graph-replayed trunk (fast True), with the trunk in
    channels-last (the default) and NCHW memory format; the train-mode case (batch statistics) on
    the module path.  Tolerance 2e-5 of the latent's range (MIOpen vs CPU convolution order) and
    latent_scaling exact."""
    import json
    import os

    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_fw.npz")))
    cases = json.loads(bytes(g["cases"]).decode())
    imgs = torch.from_numpy(g["images"]).to(DEV)
    for i, c in enumerate(cases):
        if c["train"] and fast:
            continue   # the folded trunk is eval-only
        conf = model_conf()
        conf["encoder"] = dict(backbone="resnet34", pretrained=False, num_layers=c["num_layers"],
                               feature_scale=c["feature_scale"], use_first_pool=c["use_first_pool"])
        net = PixelNeRFNet(conf)
        net.encoder.model.load_state_dict(synth.encoder_state(int(g["weight_seed"]), net.encoder.model.state_dict()))
        if layout == "nchw":
            net.encoder.model.to(memory_format=torch.contiguous_format)
        net = net.to(DEV)
        net.train(c["train"])
        net.encoder.infer_fast = fast
        x = imgs if c["train"] else imgs[:1]
        poses = synth.srn_poses([0.0] * x.shape[0]).to(DEV)
        with torch.no_grad():
            net.encode(x, poses, torch.tensor(30.0, device=DEV))
        lat = net.encoder.latent.detach().cpu()
        ref = torch.from_numpy(g["latent_%d" % i])
        assert lat.shape == ref.shape, (c, lat.shape)
        scale = float(ref.abs().max())
        d = float((lat - ref).abs().max())
        assert d <= (5e-5 if c["train"] else 2e-5) * scale, (c, fast, layout, d, scale)
        assert torch.equal(net.encoder.latent_scaling.cpu(), torch.from_numpy(g["latent_scaling_%d" % i])), c
        # the channels-last copy the ray march gathers from is the same latent
        assert torch.equal(net.encoder.latent_cl.cpu(), lat.permute(0, 2, 3, 1)), c
