"""The lean instantiation of the fused point model (``k_point_mlp<.., LEAN>``) on an MI355X
(``-m gpu``): bit identity with the general kernel and the launcher's routing.

``launch_point_mlp`` takes the lean kernel for a render of ONE source view on the projected
latent by a per-pass fused march (modes 1 and 2) without an activation save, in f16x3 or f16;
``pnr_mlp_set_lean(0)`` sends the same launches to the general kernel and ``pnr_mlp_last_kernel``
names the kernel the last launch took.  The lean kernel removes the paths such a launch never
takes and makes the tile index, the ray and the camera row scalar; every per-lane operation is
the general kernel's, so the outputs must be equal bit for bit: no tolerance.

Scene: NMR geometry (64 x 64 pixels, cameras at radius 2.7, near / far 1.2 / 4.0) on a 32 x 32
latent, rays hashed over the whole image, so points outside the latent (border clamp) occur.
"""
import pytest
import torch

import test_gpu_parity as tgp
from pnr import _lib, synth, torchops
from pnr.models import PixelNeRFNet
from pnr.renderer import NeRFRenderer

pytestmark = pytest.mark.gpu
DEV = tgp.DEV
KC, KF = 64, 64
GENERAL, LEAN = _lib.MLP_KERNEL_GENERAL, _lib.MLP_KERNEL_LEAN


def make_net(precision="f16x3", latent_proj=True):
    net = PixelNeRFNet(tgp.model_conf())
    net.load_state_dict(synth.pixelnerf_state(1), strict=False)
    net.mlp_precision = precision
    net.use_latent_proj = latent_proj
    return net.to(DEV).eval()


def encode_nmr(net, sc, n_views=1):
    lat, poses = sc["latent"], sc["poses"]
    if n_views > 1:
        lat = synth.latent(3, n_views, 512, 32, 32)
        poses = synth.srn_poses([20.0 * i for i in range(n_views)], phi=-20.0, radius=2.7)
    net.encode_latent(lat.to(DEV), poses.reshape(1, n_views, 4, 4).to(DEV), sc["focal"].to(DEV), (64, 64),
                      num_objs=1)


def render(net, rays, mode, streams, order):
    """One torch.ops.pnr.render_rays call: (c_rgb, c_depth, c_w, f_rgb, f_depth, f_w, z_c, z_f) and
    the kernel its last point-model launch took."""
    ops_ = torchops.load()
    desc, pc = net.hip_mlp(True)
    pf = net.hip_mlp(False)[1]
    u = [None] * 4 if streams is None else [t.to(DEV).contiguous() for t in streams]
    n = rays.shape[0]
    res = ops_.render_rays(*torchops.scene_args(net), torchops.desc_list(desc), pc, pf, net.hip_proj(True),
                           net.hip_proj(False), rays, n, KC, KF, 0, 0.01, True, False, u[0], u[1], u[2], u[3],
                           1234, 0, True, True, [], mode, order)
    torch.cuda.synchronize()
    return res, _lib.load().pnr_mlp_last_kernel()


@pytest.mark.parametrize("n_rays", [1, 37, 300])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_lean_kernel_is_bit_identical(precision, n_rays):
    """rgb, depth, weights and z of both passes with the switch on equal those with it off, bit for
    bit: 1, 37 and 300 rays x (64 + 64) samples (300 rays: 600 fine tiles, more than the
    workgroups, so the persistent loop and the claim path both run), ray_order absent and a
    permutation with one out-of-range entry, counter and injected draws, march modes 1 and 2."""
    sc = synth.scene_nmr(seed=3, n_rays=n_rays)
    net = make_net(precision)
    encode_nmr(net, sc)
    rays = sc["rays"].to(DEV).contiguous()
    perm = torch.randperm(n_rays, generator=torch.Generator().manual_seed(5)).to(torch.int32)
    # one out-of-range entry: that unit marches its own index, so it sits at a fixed point of the
    # permutation (every ray is still marched exactly once)
    j = n_rays // 2
    perm[int((perm == j).nonzero()[0])] = perm[j]
    perm[j] = n_rays + 7
    names = ("c_rgb", "c_depth", "c_w", "f_rgb", "f_depth", "f_w", "z_c", "z_f")
    for order in (None, perm.to(DEV)):
        for streams in (None, synth.rng_streams(11, n_rays, KC, KF, 0)):
            for mode in (1, 2):
                with _lib.lean_mlp(True):
                    on, k_on = render(net, rays, mode, streams, order)
                with _lib.lean_mlp(False):
                    off, k_off = render(net, rays, mode, streams, order)
                assert (k_on, k_off) == (LEAN, GENERAL), (k_on, k_off)
                for nm, x, y in zip(names, on, off):
                    assert x.shape == y.shape and x.numel() > 0, nm
                    assert torch.equal(x, y), (nm, mode, order is not None, streams is not None,
                                               float((x - y).abs().max()))
                assert bool(torch.isfinite(on[3]).all())


def test_routing_other_descriptors_take_the_general_kernel():
    """ns = 3, the activation save, march modes 3 and 0, a point query, fp32 / bf16x6 / bf16x9 and the
    latent-gather path all take the general kernel with the switch on (its default)."""
    lib = _lib.load()
    assert lib.pnr_mlp_set_lean(1) == 1   # default on
    sc = synth.scene_nmr(seed=3, n_rays=37)
    rays = sc["rays"].to(DEV).contiguous()

    def last_after(net, mode, n_views=1):
        encode_nmr(net, sc, n_views)
        r = NeRFRenderer(n_coarse=KC, n_fine=KF, white_bkgd=True)
        r.march_mode = mode
        with torch.no_grad():
            out = r(net, rays[None])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.fine.rgb).all())
        return lib.pnr_mlp_last_kernel()

    net = make_net()
    assert last_after(net, 2) == LEAN and last_after(net, 1) == LEAN   # the positive cases
    assert last_after(net, 3) == GENERAL      # the single-launch march
    assert last_after(net, 0) == GENERAL      # the separate kernels
    assert last_after(make_net(), 2, n_views=3) == GENERAL
    for precision in ("fp32", "bf16x6", "bf16x9"):
        assert last_after(make_net(precision), 2) == GENERAL, precision
    assert last_after(make_net(latent_proj=False), 2) == GENERAL   # the latent-gather path
    # a point query
    net = make_net()
    encode_nmr(net, sc)
    xyz = torch.from_numpy(synth.hash_sym(77, (1, 100, 3), 0.5)).to(DEV)
    vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(78, (1, 100, 3), 1.0)), dim=-1).to(DEV)
    with torch.no_grad():
        assert last_after(net, 2) == LEAN
        net(xyz, coarse=True, viewdirs=vd)
    torch.cuda.synchronize()
    assert lib.pnr_mlp_last_kernel() == GENERAL
    # the activation save: the training forward (a render under autograd)
    net = make_net(latent_proj=False).train()
    lat = sc["latent"].to(DEV).requires_grad_(True)
    net.encode_latent(lat, sc["poses"].reshape(1, 1, 4, 4).to(DEV), sc["focal"].to(DEV), (64, 64), num_objs=1)
    r = NeRFRenderer(n_coarse=KC, n_fine=KF, white_bkgd=True).to(DEV).train()
    assert last_after(make_net(), 2) == LEAN
    out = r(net, rays[None])
    torch.cuda.synchronize()
    assert out.fine.rgb.requires_grad and lib.pnr_mlp_last_kernel() == GENERAL
    # the torch ops reach the same switch
    ops_ = torchops.load()
    assert ops_.mlp_set_lean(False) == 1 and ops_.mlp_set_lean(True) == 0
    assert ops_.mlp_last_kernel() == GENERAL
