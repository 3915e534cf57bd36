"""The ray march's backward kernels against fp64 autograd of the oracle (``-m gpu``).

``pnr_composite_backward`` (``k_composite_bwd<1..4>``, K <= 256) and
``pnr_points_input_backward_masked`` (``k_points_in_bwd``) are otherwise seen only through the
parameter gradients of two end-to-end training steps (tests/test_gpu_train.py).  Here each is
called directly with random upstream gradients and compared with ``torch.autograd.grad`` through
``oracle/ref_cpu.py`` on fp64 copies of the same inputs.

Tolerance.  No constant: the yardstick is the fp32 CPU autograd of the same function against the
fp64 one, per gradient tensor, as max |error| / max |fp64 gradient|, pooled as the maximum over
the cases of a kernel; the kernel must stay within MARGIN = 4 times it in the same norm.  The
kernels sum in another order than torch (wave trees, a suffix sum taken as total minus prefix,
run-wise accumulation and atomics) with the device's expf / cosf, so their error is another draw
from the same population rather than the same rounding sequence; a wrong neighbour, lane
boundary or missing term shows at 1e-2 or more.  Every test prints the yardstick and the
kernel's figure.  No ray, sample or point is excluded from any comparison.
"""
import functools

import pytest
import torch

from oracle import ref_cpu
from pnr import _lib, synth
from pnr.models import PixelNeRFNet
from test_gpu_train import conf

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 4.0


def rel_err(a, ref):
    """max |a - ref| / max |ref| in fp64."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


# ------------------------------------------------------ composite backward --
# every S = ceil(K / 64) and both sides of every lane-ownership boundary (lane l owns samples
# S l .. S l + S - 1)
BWD_K = [1, 2, 63, 64, 65, 96, 127, 128, 129, 192, 193, 255, 256]
BWD_B = 13   # not a multiple of the 4 rays of a block
NEAR, FAR = 0.3, 4.0


def composite_bwd_inputs(K, white):
    """Inputs as test_gpu_parity.test_composite_matches_oracle_random with rows 0-5 edge rows:
    0 sigma all -1 (nothing absorbs); 1 sigma all exactly 0 (the relu kink: gradient 0 on both
    sides of this comparison); 2 sigma all 400 (exp underflows where delta is large enough, so
    s_i = 1e-10); 3 z[3, 1] = z[3, 0], a zero delta; 4 z[4, -1] = far, a zero last delta;
    5 one sample with sigma 1e4 in mid-ray (everything behind it is hidden)."""
    g = torch.Generator().manual_seed(7000 + 2 * K + int(white))
    B = BWD_B
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), NEAR), torch.full((B, 1), FAR)], 1)
    z = torch.sort(NEAR + (FAR - NEAR) * torch.rand(B, K, generator=g), -1)[0]
    raw = torch.rand(B, K, 4, generator=g)
    raw[..., 3] = torch.randn(B, K, generator=g) * 4.0
    raw[0, :, 3] = -1.0
    raw[1, :, 3] = 0.0
    raw[2, :, 3] = 400.0
    if K > 1:
        z[3, 1] = z[3, 0]
    z[4, -1] = FAR
    raw[5, K // 2, 3] = 1e4
    d_rgb = torch.randn(B, 3, generator=g)
    d_depth = torch.randn(B, generator=g)
    d_w = torch.randn(B, K, generator=g)
    return dict(rays=rays, z=z, raw=raw, d_rgb=d_rgb, d_depth=d_depth, d_w=d_w, white=white, K=K)


def composite_autograd(c, dtype, use_w=True, use_depth=True):
    """(d_raw, d_z) = autograd of sum(w d_w) + sum(rgb d_rgb) + sum(depth d_depth) through
    ref_cpu.composite in ``dtype``."""
    z = c["z"].clone().to(dtype).requires_grad_(True)   # clone: the inputs are shared and stay plain
    raw = c["raw"].clone().to(dtype).requires_grad_(True)
    w, rgb, depth = ref_cpu.composite(c["rays"].to(dtype), z, raw, c["white"])
    loss = (rgb * c["d_rgb"].to(dtype)).sum()
    if use_w:
        loss = loss + (w * c["d_w"].to(dtype)).sum()
    if use_depth:
        loss = loss + (depth * c["d_depth"].to(dtype)).sum()
    return torch.autograd.grad(loss, (raw, z))


@functools.lru_cache(maxsize=None)
def composite_bwd_reference():
    """The inputs and fp64 gradients of every (K, white) case, and the pooled yardstick per
    tensor: the maximum over all of them of the fp32 CPU autograd's error in rel_err's norm."""
    cases, pooled = {}, dict(d_raw=0.0, d_z=0.0)
    for K in BWD_K:
        for white in (False, True):
            c = composite_bwd_inputs(K, white)
            c["ref"] = composite_autograd(c, torch.float64)
            f32 = composite_autograd(c, torch.float32)
            for name, a, b in zip(("d_raw", "d_z"), f32, c["ref"]):
                assert torch.isfinite(a).all() and torch.isfinite(b).all(), (K, white, name)
                pooled[name] = max(pooled[name], rel_err(a, b))
            cases[(K, white)] = c
    return cases, pooled


def run_composite_bwd(c, d_depth=True, d_w=True, want_dz=True, prefill=float("nan")):
    """pnr_composite_backward through the C ABI into pre-filled outputs; returns (status, d_raw,
    d_z)."""
    B, K = c["z"].shape
    dev = lambda t: t.to(DEV).contiguous()   # noqa: E731
    z, raw, rays, d_rgb = dev(c["z"]), dev(c["raw"]), dev(c["rays"]), dev(c["d_rgb"])
    gd = dev(c["d_depth"]) if d_depth else None
    gw = dev(c["d_w"]) if d_w else None
    d_raw = torch.full((B, K, 4), prefill, device=DEV)
    d_z = torch.full((B, K), prefill, device=DEV) if want_dz else None
    lib = _lib.load()
    rc = lib.pnr_composite_backward(_lib.ptr(z), _lib.ptr(raw), _lib.ptr(rays), B, K, int(c["white"]),
                                    _lib.ptr(d_rgb), _lib.ptr(gd), _lib.ptr(gw), _lib.ptr(d_raw), _lib.ptr(d_z),
                                    _lib.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, d_raw, d_z


def check_against(what, got, ref, pooled):
    for name, a, b in zip(("d_raw", "d_z"), got, ref):
        if a is None:
            continue
        assert torch.isfinite(a).all(), "%s: %s not finite" % (what, name)
        e = rel_err(a, b)
        print("%s %s: fp32-vs-fp64 yardstick %.3g, kernel %.3g, ratio %.2f" % (
            what, name, pooled[name], e, e / pooled[name]))
        assert e <= MARGIN * pooled[name], "%s %s: kernel error %.3g > %g x yardstick %.3g" % (
            what, name, e, MARGIN, pooled[name])


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("K", BWD_K)
def test_composite_backward_matches_fp64_autograd(K, white):
    cases, pooled = composite_bwd_reference()
    c = cases[(K, white)]
    rc, d_raw, d_z = run_composite_bwd(c)
    assert rc == 0, _lib.load().pnr_last_error()
    check_against("composite backward K=%d white=%d" % (K, white), (d_raw, d_z), c["ref"], pooled)


def test_composite_backward_optional_gradients():
    """d_weights = NULL and d_depth = NULL drop their term; d_z = NULL leaves d_raw unchanged."""
    cases, pooled = composite_bwd_reference()
    c = cases[(96, True)]
    rc, d_raw_full, _ = run_composite_bwd(c)
    assert rc == 0
    rc, d_raw, d_z = run_composite_bwd(c, d_w=False)
    assert rc == 0
    check_against("composite backward d_weights=NULL", (d_raw, d_z),
                  composite_autograd(c, torch.float64, use_w=False), pooled)
    rc, d_raw, d_z = run_composite_bwd(c, d_depth=False)
    assert rc == 0
    check_against("composite backward d_depth=NULL", (d_raw, d_z),
                  composite_autograd(c, torch.float64, use_depth=False), pooled)
    rc, d_raw, d_z = run_composite_bwd(c, want_dz=False)
    assert rc == 0 and d_z is None
    assert torch.equal(d_raw, d_raw_full)
    check_against("composite backward d_z=NULL", (d_raw, None), c["ref"], pooled)


def test_composite_backward_refuses_k_above_256_and_takes_no_rays():
    c = composite_bwd_inputs(257, True)
    rc, d_raw, d_z = run_composite_bwd(c, prefill=-7.0)
    assert rc == -2, rc   # PNR_ERR_UNSUPPORTED
    assert bool((d_raw == -7.0).all()) and bool((d_z == -7.0).all())
    c = composite_bwd_inputs(96, True)
    for k in ("rays", "z", "raw", "d_rgb", "d_depth", "d_w"):
        c[k] = c[k][:0]
    rc, d_raw, d_z = run_composite_bwd(c)
    assert rc == 0 and d_raw.shape == (0, 96, 4)


# ---------------------------------------------------- input-stage backward --
H_L, W_L = 12, 14        # the small latent of tests/test_gpu_train.py::case
IMG_W, IMG_H = 400, 300
INT_GUARD = 1e-3         # no point this close to an integer latent coordinate (the bilinear kink)
CAM_GUARD = 0.3          # nor this close to a source camera's plane (the projection's pole)
EDGE_CLASSES = {"left", "right", "top", "bottom", "behind", "inside"}


def input_stage_scene(sb, ns, seed):
    sc = synth.scene_multiview(seed=seed, n_views=sb * ns, n_rays=1, channels=512, h_l=H_L, w_l=W_L)
    assert (sc["width"], sc["height"]) == (IMG_W, IMG_H)
    focal = torch.tensor([[300.0, 310.0], [290.0, 295.0]])[:sb]
    c = torch.tensor([[195.0, 152.0], [200.0, 148.0]])[:sb]
    return dict(latent=sc["latent"], poses=sc["poses"].reshape(sb, ns, 4, 4), focal=focal, c=c, sb=sb, ns=ns)


def latent_coords(sn, rays, z):
    """fp64 unclipped latent pixel coordinates (ix, iy) and camera-space depth of every point
    o + z d of rays (sb, rpo, 8) in every source view of its object: each (sb, ns, rpo * K)."""
    sb, ns = sn["sb"], sn["ns"]
    poses_wc, focal, c, _, _ = ref_cpu.encode_buffers(sn["poses"], sn["focal"], IMG_W, IMG_H, sn["c"])
    poses_wc = poses_wc.double().reshape(sb, ns, 3, 4)
    r = rays.double()
    pts = (r[:, :, None, :3] + z.double().unsqueeze(-1) * r[:, :, None, 3:6]).reshape(sb, 1, -1, 3)
    cam = torch.matmul(poses_wc[:, :, None, :, :3], pts.unsqueeze(-1))[..., 0] + poses_wc[:, :, None, :, 3]
    uv = -cam[..., :2] / cam[..., 2:] * focal.double()[:, None, None, :] + c.double()[:, None, None, :]
    return uv[..., 0] * W_L / IMG_W, uv[..., 1] * H_L / IMG_H, cam[..., 2]


def input_stage_rays(sn, rpo, K, seed):
    """rpo rays per object with K sorted depths each, chosen from random candidates (origin
    U(-3, 3)^3, unit direction towards a point near the scene centre, depths U(0.1, 5)):
    a candidate is re-drawn when a point of it lies within INT_GUARD of an integer latent
    coordinate or of 0 / W - 1 / H - 1 in a source view (bilinear sampling is not differentiable
    there) or within CAM_GUARD of a source camera's plane.  The first rays taken are ones that
    add an edge class not yet present -- points projecting off the image on the left / right /
    top / bottom, points behind a camera, points inside the image -- and all six must be
    present.  This is input construction: every point of every ray taken is compared."""
    g = torch.Generator().manual_seed(seed)
    sb = sn["sb"]
    chosen, have = [[] for _ in range(sb)], set()
    for _ in range(4000):
        if all(len(ch) == rpo for ch in chosen):
            break
        o = (torch.rand(sb, 1, 3, generator=g) * 2.0 - 1.0) * 3.0
        tgt = (torch.rand(sb, 1, 3, generator=g) * 2.0 - 1.0) * 0.8
        d = torch.nn.functional.normalize(tgt - o, dim=-1)
        ray = torch.cat([o, d, torch.full((sb, 1, 1), 0.1), torch.full((sb, 1, 1), 5.0)], -1)
        zz = torch.sort(0.1 + 4.9 * torch.rand(sb, 1, K, generator=g), -1)[0]
        ix, iy, cz = latent_coords(sn, ray, zz)
        for s in range(sb):
            if len(chosen[s]) == rpo:
                continue
            x, y, depth = ix[s], iy[s], cz[s]
            kink = ((x - x.round()).abs().min() < INT_GUARD or (y - y.round()).abs().min() < INT_GUARD
                    or depth.abs().min() < CAM_GUARD)
            if kink:
                continue
            front = depth < 0
            inside = front & (x > 0) & (x < W_L - 1) & (y > 0) & (y < H_L - 1)
            classes = {n for n, m in (("left", front & (x < 0)), ("right", front & (x > W_L - 1)),
                                      ("top", front & (y < 0)), ("bottom", front & (y > H_L - 1)),
                                      ("behind", ~front), ("inside", inside)) if bool(m.any())}
            slots_left = sum(rpo - len(ch) for ch in chosen)
            missing = EDGE_CLASSES - have
            if missing and len(classes & missing) * slots_left < len(missing):
                continue   # each ray taken adds its share of the classes still missing
            if not missing and int(inside.sum()) < K // 2:
                continue   # once every class is present, take rays that cross the image
            have |= classes
            chosen[s].append((ray[s, 0], zz[s, 0]))
    assert all(len(ch) == rpo for ch in chosen), [len(ch) for ch in chosen]
    assert have == EDGE_CLASSES, have
    rays = torch.stack([torch.stack([r for r, _ in ch]) for ch in chosen])     # (sb, rpo, 8)
    z = torch.stack([torch.stack([zz for _, zz in ch]) for ch in chosen])       # (sb, rpo, K)
    return rays, z


def input_stage_autograd(sn, sd, rays, z, d_feat, d_zlat, dtype):
    """(d_latent channels-last (sb ns, H, W, 512), d_z (sb rpo K)) = autograd of
    sum(z_feature d_feat[:, :42]) + sum(latent_rows d_zlat) through ref_cpu.pixelnerf_input_stage
    at the points o + z d, in ``dtype``.  d_feat / d_zlat rows are the kernel's: view-major,
    v * n_points + p."""
    sb, ns = sn["sb"], sn["ns"]
    rpo, K = z.shape[1], z.shape[2]
    latent = sn["latent"].clone().to(dtype).requires_grad_(True)   # clone: the inputs stay plain
    zz = z.clone().to(dtype).requires_grad_(True)
    scene = ref_cpu.Scene(latent, sn["poses"], sn["focal"], IMG_W, IMG_H, sn["c"])
    for k in ("poses", "focal", "c", "image_shape"):
        setattr(scene, k, getattr(scene, k).to(dtype))
    sdd = {k: v.to(dtype) for k, v in sd.items() if k.startswith("code.")}
    r = rays.to(dtype)
    pts = (r[:, :, None, :3] + zz.unsqueeze(-1) * r[:, :, None, 3:6]).reshape(sb, rpo * K, 3)
    dirs = r[:, :, None, 3:6].expand(-1, -1, K, -1).reshape(sb, rpo * K, 3)
    lat_rows, feat = ref_cpu.pixelnerf_input_stage(sdd, scene, pts, dirs)

    def oracle_rows(t):   # (view, object, point) rows -> the oracle's (object, view, point)
        return t.to(dtype).reshape(ns, sb, rpo * K, -1).transpose(0, 1).reshape(sb * ns * rpo * K, -1)

    loss = (feat * oracle_rows(d_feat)[:, :42]).sum() + (lat_rows * oracle_rows(d_zlat)).sum()
    g_lat, g_z = torch.autograd.grad(loss, (latent, zz))
    return g_lat.permute(0, 2, 3, 1).contiguous(), g_z.reshape(-1)


INPUT_CASES = {
    # NS = 1, n_points = 3 * 41 = 123: no multiple of the 8-point run nor of 4 waves x 8
    "ns1": dict(sb=1, ns=1, rpo=3, K=41, seed=11),
    # SB = 2 objects x NS = 3 views, 6 rays per object, K = 7
    "ns3": dict(sb=2, ns=3, rpo=6, K=7, seed=12),
}


@functools.lru_cache(maxsize=None)
def input_stage_reference():
    """Inputs and fp64 gradients of INPUT_CASES, and the pooled yardstick per tensor (d_latent,
    d_z): the maximum over the cases of the fp32 CPU autograd's error in rel_err's norm."""
    cases, pooled = {}, dict(d_latent=0.0, d_z=0.0)
    sd = synth.pixelnerf_state(5)
    for name, p in INPUT_CASES.items():
        sn = input_stage_scene(p["sb"], p["ns"], p["seed"])
        rays, z = input_stage_rays(sn, p["rpo"], p["K"], p["seed"] + 100)
        n_points = p["sb"] * p["rpo"] * p["K"]
        g = torch.Generator().manual_seed(p["seed"] + 200)
        d_feat = torch.randn(p["ns"] * n_points, 64, generator=g)
        d_zlat = torch.randn(p["ns"] * n_points, 512, generator=g)
        ref = input_stage_autograd(sn, sd, rays, z, d_feat, d_zlat, torch.float64)
        f32 = input_stage_autograd(sn, sd, rays, z, d_feat, d_zlat, torch.float32)
        per_case = {}
        for tn, a, b in zip(("d_latent", "d_z"), f32, ref):
            assert torch.isfinite(a).all() and torch.isfinite(b).all(), (name, tn)
            per_case[tn] = rel_err(a, b)
            pooled[tn] = max(pooled[tn], per_case[tn])
        # latent pixels a point's (clipped) bilinear footprint touches, per (image, y, x)
        ix, iy, _ = latent_coords(sn, rays, z)
        x0 = ix.clamp(0, W_L - 1).floor().long()
        y0 = iy.clamp(0, H_L - 1).floor().long()
        touched = torch.zeros(p["sb"] * p["ns"], H_L, W_L, dtype=torch.bool)
        img = torch.arange(p["sb"] * p["ns"]).reshape(p["sb"], p["ns"], 1).expand_as(x0)
        for dy in (0, 1):
            for dx in (0, 1):
                touched[img, (y0 + dy).clamp_max(H_L - 1), (x0 + dx).clamp_max(W_L - 1)] = True
        cases[name] = dict(p, sn=sn, sd=sd, rays=rays, z=z, d_feat=d_feat, d_zlat=d_zlat, ref=ref,
                           touched=touched, n_points=n_points, yardstick=per_case)
    return cases, pooled


def run_input_bwd(c, want_latent=True, want_dz=True, mask=None):
    """pnr_points_input_backward_masked through the C ABI on case ``c``: (d_latent, d_z)."""
    sn = c["sn"]
    net = PixelNeRFNet(conf())
    net.load_state_dict(c["sd"], strict=False)
    net = net.to(DEV)
    net.encode_latent(sn["latent"].to(DEV), sn["poses"].to(DEV), sn["focal"].to(DEV), (IMG_W, IMG_H),
                      c=sn["c"].to(DEV), num_objs=sn["sb"])
    desc, packed = net.mlp_coarse.packed(net.code, "fp32")
    rays = c["rays"].reshape(-1, 8).to(DEV).contiguous()
    z = c["z"].reshape(rays.shape[0], c["K"]).to(DEV).contiguous()
    d_feat, d_zlat = c["d_feat"].to(DEV).contiguous(), c["d_zlat"].to(DEV).contiguous()
    d_lat = torch.zeros_like(net.encoder.latent_cl) if want_latent else None
    d_z = torch.full((c["n_points"],), float("nan"), device=DEV) if want_dz else None
    zm = mask.to(device=DEV, dtype=torch.uint8).contiguous() if mask is not None else None
    r = _lib.Rays(_lib.ptr(rays), rays.shape[0], c["rpo"])
    lib = _lib.load()
    _lib.check(lib.pnr_points_input_backward_masked(
        net.hip_scene(), desc, _lib.ptr(packed), r, _lib.ptr(z), c["K"], _lib.ptr(d_feat), _lib.ptr(d_zlat),
        _lib.ptr(d_lat), _lib.ptr(d_z), _lib.ptr(zm), _lib.stream_of(torch.device(DEV))),
        "pnr_points_input_backward_masked")
    torch.cuda.synchronize()
    return d_lat, d_z


def check_input(what, c, pooled, d_lat, d_z, mask=None):
    ref_lat, ref_z = c["ref"]
    if mask is not None:
        ref_z = ref_z * mask.to(ref_z.dtype)
    for name, a, b in (("d_latent", d_lat, ref_lat), ("d_z", d_z, ref_z)):
        if a is None:
            continue
        assert torch.isfinite(a).all(), "%s: %s not finite" % (what, name)
        e = rel_err(a, b)
        print("%s %s: fp32-vs-fp64 yardstick %.3g (this case alone %.3g), kernel %.3g, ratio %.2f" % (
            what, name, pooled[name], c["yardstick"][name], e, e / pooled[name]))
        assert e <= MARGIN * pooled[name], "%s %s: kernel error %.3g > %g x yardstick %.3g" % (
            what, name, e, MARGIN, pooled[name])
    if d_lat is not None:
        # a latent pixel outside every point's footprint receives nothing at all
        assert bool(c["touched"].any()) and not bool(c["touched"].all())
        assert float(d_lat.cpu()[~c["touched"]].abs().max()) == 0.0, what


@pytest.mark.parametrize("name", sorted(INPUT_CASES))
def test_points_input_backward_matches_fp64_autograd(name):
    cases, pooled = input_stage_reference()
    c = cases[name]
    d_lat, d_z = run_input_bwd(c)
    check_input("input backward %s" % name, c, pooled, d_lat, d_z)


@pytest.mark.parametrize("name", sorted(INPUT_CASES))
def test_points_input_backward_z_mask_and_optional_outputs(name):
    """z_mask: d_z exactly 0 where the mask is 0 and the unmasked value elsewhere, d_latent
    unchanged (up to its atomics' order).  d_latent = NULL leaves d_z unchanged; d_z = NULL
    leaves d_latent unchanged."""
    cases, pooled = input_stage_reference()
    c = cases[name]
    d_lat0, d_z0 = run_input_bwd(c)
    mask = torch.from_numpy(synth.hash_uniform(31, c["n_points"]) < 0.4)
    assert bool(mask.any()) and not bool(mask.all())
    d_lat, d_z = run_input_bwd(c, mask=mask)
    assert float(d_z[~mask.to(DEV)].abs().max()) == 0.0
    assert torch.equal(d_z[mask.to(DEV)], d_z0[mask.to(DEV)])
    check_input("input backward %s z_mask" % name, c, pooled, d_lat, d_z, mask=mask)
    d_lat, d_z = run_input_bwd(c, want_latent=False)
    assert d_lat is None and torch.equal(d_z, d_z0)
    d_lat, d_z = run_input_bwd(c, want_dz=False)
    assert d_z is None
    check_input("input backward %s d_z=NULL" % name, c, pooled, d_lat, None)
