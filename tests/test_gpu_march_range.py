"""The along-ray forward kernels over their whole K range (``-m gpu``).

``pnr_composite`` takes any K and ``pnr_sample_fine`` / the render take n_coarse + n_fine <= 1024;
tests/test_gpu_parity.py stops at K = 200 / 228 / 192.  Here every composite kernel
(``k_composite_c<1..4>`` and the chunked ``k_composite`` for K > 256) runs at both sides of its K
range with ray counts that end inside a two-rays-per-wave pair and inside a four-wave block, the
samplers run up to 1024 samples (the 64-sample cdf carry chunks, the LDS bitonic sort at
n_sort = 256 / 512 / 1024 and its padding with infinities), and one render has 288 samples per ray.

No ray or sample is excluded from a comparison, except by the flip classification
``compare_render`` (tests/test_gpu_parity.py) applies to the render under its MAX_FLIPS.
"""
import pytest
import torch

from oracle import parity, ref_cpu
from pnr import _lib, ops, synth
from pnr.models import PixelNeRFNet
from pnr.renderer import NeRFRenderer
from test_gpu_parity import assert_close, compare_render, model_conf

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, K) by the kernel launch_composite picks: S = ceil(K / 64) <= 4 -> k_composite_c<S>, two rays
# per wave; K > 256 -> k_composite, one ray per wave.  Odd B: the pair tail b0 + 1 >= n_rays and
# a last block with fewer than four waves at work.
COMPOSITE_CASES = [
    (1, 1), (2, 63), (7, 64),                                          # S = 1
    (9, 65), (66, 128),                                                # S = 2
    (1, 129), (67, 192),                                               # S = 3
    (5, 193), (13, 256),                                               # S = 4
    (1, 257), (9, 257), (66, 300), (5, 320), (13, 511), (7, 1024),     # generic kernel
]
NULL_WEIGHT_CASES = [(7, 64), (9, 65), (67, 192), (13, 256), (9, 257)]   # one per kernel family


def composite_inputs(B, K):
    """As test_gpu_parity.test_composite_matches_oracle_random: sorted uniform depths in
    (near, far), rgb U(0, 1), sigma 4 N(0, 1).  The fp32 oracle is within 2.2e-7 of its own fp64
    evaluation on these for K up to 1024, and the weights past sample 256 reach 1e-2."""
    g = torch.Generator().manual_seed(1000 * K + B)
    near, far = 0.3, 4.0
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), near), torch.full((B, 1), far)], 1)
    z = torch.sort(near + (far - near) * torch.rand(B, K, generator=g), -1)[0]
    raw = torch.rand(B, K, 4, generator=g)
    raw[..., 3] = torch.randn(B, K, generator=g) * 4.0
    return rays, z, raw


def abi_composite(rays, z, raw, white, want_weights=True):
    """pnr_composite through the C ABI into NaN-filled outputs: a row the kernel does not write
    stays NaN and fails the comparison whatever the allocator returned."""
    B, K = z.shape
    rays, z, raw = rays.to(DEV), z.to(DEV), raw.to(DEV)
    nan = float("nan")
    w = torch.full((B, K), nan, device=DEV) if want_weights else None
    rgb = torch.full((B, 3), nan, device=DEV)
    d = torch.full((B,), nan, device=DEV)
    lib = _lib.load()
    _lib.check(lib.pnr_composite(_lib.ptr(z), _lib.ptr(raw), _lib.ptr(rays), B, K, int(white), _lib.ptr(w),
                                 _lib.ptr(rgb), _lib.ptr(d), _lib.stream_of(torch.device(DEV))), "pnr_composite")
    torch.cuda.synchronize()
    return w, rgb, d


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("B,K", COMPOSITE_CASES)
def test_composite_every_kernel_and_tail(B, K, white):
    rays, z, raw = composite_inputs(B, K)
    w_ref, rgb_ref, d_ref = ref_cpu.composite(rays, z, raw, white)
    w, rgb, d = abi_composite(rays, z, raw, white)
    what = "B=%d K=%d white=%d" % (B, K, white)
    assert_close(w, w_ref, "weights " + what)
    assert_close(rgb, rgb_ref, "rgb " + what)
    assert_close(d, d_ref, "depth " + what)


@pytest.mark.parametrize("B,K", NULL_WEIGHT_CASES)
def test_composite_without_weights_is_bit_identical(B, K):
    rays, z, raw = composite_inputs(B, K)
    _, rgb0, d0 = abi_composite(rays, z, raw, True)
    w1, rgb1, d1 = abi_composite(rays, z, raw, True, want_weights=False)
    assert w1 is None
    assert torch.isfinite(rgb0).all() and torch.isfinite(d0).all()
    assert torch.equal(rgb0, rgb1) and torch.equal(d0, d1)


# ---------------------------------------------------------------- samplers --
@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("B,K", [(3, 256), (3, 257), (2, 1024)])
def test_sample_coarse_up_to_1024(B, K, lindisp):
    g = torch.Generator().manual_seed(K)
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), 0.8), torch.full((B, 1), 1.8)], 1)
    u = torch.rand(B, K, generator=g)
    ref = ref_cpu.sample_coarse(rays, K, u, lindisp)
    z = ops.sample_coarse(rays.to(DEV), K, u.to(DEV), lindisp)
    assert_close(z, ref, "z_coarse K=%d lindisp=%d" % (K, lindisp), atol=2e-6, rtol=2e-6)


def draws_off_the_cdf(u, w, guard=4e-6, step=1.2e-5):
    """``u`` with every draw within ``guard`` of an entry of the cdf of ``w`` (parity.fine_cdf)
    moved by ``step`` modulo 1, repeated until none is left.  searchsorted is discontinuous at the
    cdf entries and the device sums the pdf normaliser in another order than torch, so a draw ON
    an entry may take either bin; away from them both must agree, and no ray is excluded."""
    cdf = parity.fine_cdf(w)
    u = u.clone()
    moved = 0
    for _ in range(100):
        idx = torch.searchsorted(cdf, u.contiguous(), right=True).clamp(1, cdf.shape[1] - 1)
        dist = torch.minimum((u - cdf.gather(1, idx - 1)).abs(), (u - cdf.gather(1, idx)).abs())
        near = dist <= guard
        if not bool(near.any()):
            return u, moved
        moved += int(near.sum())
        u = torch.where(near, torch.remainder(u + step, 1.0), u)
    raise AssertionError("draws still within %g of a cdf entry" % guard)


@pytest.mark.parametrize("kc,kf,kfd,lindisp", [
    (256, 256, 0, False),    # n_sort 512, four full cdf chunks
    (300, 212, 20, False),   # a partial fifth cdf chunk, depth samples
    (512, 512, 0, False),    # n_sort 1024 with no padding
    (64, 960, 64, False),    # one cdf chunk, 15 rounds of draws per lane
    (960, 64, 0, False),     # 15 cdf chunks
    (129, 127, 0, False),    # n_sort 256 exactly filled, one cdf entry in the third chunk
    (1, 1023, 0, False),     # a single bin
    (300, 212, 20, True),    # lindisp
])
def test_sample_fine_up_to_1024(kc, kf, kfd, lindisp):
    g = torch.Generator().manual_seed(kc + kf)
    B = 65
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), 0.5), torch.full((B, 1), 3.5)], 1)
    zc = ref_cpu.sample_coarse(rays, kc, torch.rand(B, kc, generator=g), lindisp)
    w = torch.rand(B, kc, generator=g) ** 4
    w[:3] = 0.0                      # all-zero weights -> uniform pdf
    depth = 0.5 + 3.0 * torch.rand(B, generator=g)
    nf = kf - kfd
    u, moved = draws_off_the_cdf(torch.rand(B, nf, generator=g), w)
    uj = torch.rand(B, nf, generator=g)
    nd = torch.randn(B, kfd, generator=g)
    samps = [zc, ref_cpu.sample_fine(rays, w, kc, u, uj, lindisp)]
    if kfd > 0:
        samps.append(ref_cpu.sample_fine_depth(rays, depth, kfd, 0.01, nd))
    ref = torch.sort(torch.cat(samps, -1), -1)[0]
    zf = ops.sample_fine(rays.to(DEV), zc.to(DEV), w.to(DEV), depth.to(DEV), kf, kfd, 0.01,
                         u.to(DEV), uj.to(DEV), nd.to(DEV), lindisp).cpu()
    print("sample_fine (%d, %d, %d): %d of %d draws moved off a cdf entry" % (kc, kf, kfd, moved, u.numel()))
    assert torch.isfinite(zf).all()
    assert_close(zf, ref, "z_fine (%d, %d, %d)" % (kc, kf, kfd), 2e-6, 2e-6)


# ------------------------------------------------------------------ render --
@pytest.mark.parametrize("share", [False, True])
def test_render_with_288_samples_per_ray(share):
    """64 coarse + 224 fine (16 of them depth samples): the fused coarse pass, then the separate
    fine sampler (n_sort = 512), MLP and the chunked composite.  ``share``: mlp_fine = None, so
    the fine pass evaluates only the 224 new samples and merges the coarse pass's outputs
    (k_merge_raw, the index-carrying LDS sort)."""
    kc, kf, kfd, B = 64, 224, 16, 13
    sd = synth.pixelnerf_state(3)
    sc = synth.scene_srn(seed=4, n_rays=B, pick="hash")
    streams = synth.rng_streams(6, B, kc, kf, kfd)
    net = PixelNeRFNet(model_conf())
    net.load_state_dict(sd, strict=False)
    net.mlp_precision = "f16x3"
    sd_ref = dict(sd)
    if share:
        net.mlp_fine = None
        for k in list(sd):
            if k.startswith("mlp_fine."):
                sd_ref[k] = sd["mlp_coarse." + k[len("mlp_fine."):]]
    net = net.to(DEV).eval()
    net.encode_latent(sc["latent"].to(DEV), sc["poses"].to(DEV), sc["focal"].to(DEV), (128, 128))
    r = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True)
    r.streams = streams
    r.return_z = True
    with torch.no_grad():
        out = r(net, sc["rays"][None].to(DEV), want_weights=True)
    torch.cuda.synchronize()
    assert out.fine.weights.shape[-1] == kc + kf
    scene = ref_cpu.Scene(sc["latent"], sc["poses"], sc["focal"], 128, 128, None)
    with torch.no_grad():
        ref = ref_cpu.render(lambda p, c, d: ref_cpu.pixelnerf_forward(sd_ref, scene, p, c, d),
                             sc["rays"][None], kc, kf, kfd, streams, True)
    arr = dict(coarse_rgb=ref["coarse"]["rgb"], coarse_depth=ref["coarse"]["depth"],
               coarse_weights=ref["coarse"]["weights"], fine_rgb=ref["fine"]["rgb"],
               fine_depth=ref["fine"]["depth"], fine_weights=ref["fine"]["weights"], z_fine=ref["fine"]["z"],
               z_coarse=ref["coarse"]["z"], rays=sc["rays"], u_coarse=streams[0], u_fine=streams[1],
               u_fine_jit=streams[2], n_depth=streams[3])
    compare_render("288 samples share=%d" % share, out, dict(n_fine=kf, n_fine_depth=kfd), arr,
                   oracle=(sd_ref, scene, {}, True, B))
