"""The along-ray kernels on surface-like inputs: opaque, peaked, clustered (``-m gpu``).

Every other test of ``k_composite_c<1..4>``, ``k_composite``, ``k_sample_fine`` / ``sample_fine_wave``
and the fused epilogue of ``k_point_mlp`` feeds them noise-like data: sigma 4 N(0, 1), weights
rand**4, a synthetic model whose sigma stays below 3.3.  A ray's weight is then spread over dozens
of samples.  A trained model puts one or two opaque samples on a ray; that is where the double
transmittance carry across 64-sample chunks, the ``far`` delta of the last sample, the lane-63 to
lane-0 neighbour, the cdf carry chunks and the sorts on equal and near-equal keys do their work.
tests/march_surface.py builds such inputs (tests/test_march_surface_inputs.py keeps them honest on
the CPU); here the kernels run on them.  No ray, sample or draw is excluded from any comparison.

Tolerance of the composite.  No constant: the yardstick is fp32 ``ref_cpu.composite`` against its
own fp64 evaluation, max |error| per output tensor, pooled as the maximum over all (K, white) cases
of ``test_composite_opaque_rows``; the kernel, against fp64, must stay within MARGIN = 4 times it
(the margin of tests/test_gpu_march_backward.py: the kernel reproduces torch's double cumprod but
uses the device's expf and sums in another order), and within the suite's 5e-5 + 1e-5 |ref| anyway.
"""
import copy
import functools

import pytest
import torch

import march_surface as ms
from oracle import parity, ref_cpu
from pnr import ops, synth
from pnr.models import PixelNeRFNet
from pnr.renderer import NeRFRenderer
from test_gpu_march_range import abi_composite
from test_gpu_parity import assert_close, model_conf

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 4.0
NAMES = ("weights", "rgb", "depth")


# --------------------------------------------------------------- composite --
@functools.lru_cache(maxsize=None)
def composite_reference():
    """Inputs and fp64 results of every (K, white) case, and the pooled yardstick per tensor: the
    maximum over the cases of |fp32 ref_cpu.composite - its fp64 evaluation|."""
    cases = {}
    pooled = dict.fromkeys(NAMES, 0.0)
    for K in sorted(set(ms.COMPOSITE_KS + ms.POISON_KS)):
        rays, z, raw = ms.composite_rows(K, K)
        for white in (False, True):
            r64 = ms.composite_ref64(rays, z, raw, white)
            if K in ms.COMPOSITE_KS:
                r32 = ref_cpu.composite(rays, z, raw, white)
                for name, a, b in zip(NAMES, r32, r64):
                    pooled[name] = max(pooled[name], float((a.double() - b).abs().max()))
            cases[(K, white)] = (rays, z, raw, r64)
    print("composite yardstick (fp32 oracle vs fp64, pooled): " + ", ".join("%s %.3g" % (n, pooled[n]) for n in NAMES))
    return cases, pooled


def check_composite(what, got, r64, pooled, where=None):
    """``got`` (weights, rgb, depth) from the device against the fp64 reference, on the entries
    ``where[name]`` selects (default all): 4 x the pooled yardstick and the suite's outer bound."""
    for name, a, b in zip(NAMES, got, r64):
        a = a.detach().cpu()
        if where is not None:
            a, b = a[where[name]], b[where[name]]
        if a.numel() == 0:
            continue
        e = float((a.double() - b).abs().max())
        print("%s %s: yardstick %.3g, kernel %.3g, ratio %.2f" % (what, name, pooled[name], e, e / pooled[name]))
        assert e <= MARGIN * pooled[name], "%s %s: kernel error %.3g > %g x yardstick %.3g" % (
            what, name, e, MARGIN, pooled[name])
        assert_close(a, b.float(), "%s %s" % (what, name))


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("K", ms.COMPOSITE_KS)
def test_composite_opaque_rows(K, white):
    """Every composite kernel (S = 1 .. 4 of k_composite_c, the chunked k_composite) on the nine
    rows of ``composite_rows``: opaque samples on either side of a chunk boundary and on the last
    sample, a transmittance that underflows the double range, zero deltas under a huge sigma.
    Without the weights pointer rgb and depth are the same bits."""
    cases, pooled = composite_reference()
    rays, z, raw, r64 = cases[(K, white)]
    got = abi_composite(rays, z, raw, white)
    check_composite("K=%d white=%d" % (K, white), got, r64, pooled)
    w1, rgb1, d1 = abi_composite(rays, z, raw, white, want_weights=False)
    assert w1 is None and torch.equal(rgb1, got[1]) and torch.equal(d1, got[2])


@pytest.mark.parametrize("K", [K for K in ms.COMPOSITE_KS if K >= 2])
def test_composite_carries_the_transmittance_exactly(K):
    """The double transmittance carry, bit for bit.  An error in the low word of the carried
    double is 2^-20 of the transmittance: at most 9.5e-7, of which the fp32-level bound above sees
    only the upper half (a kernel whose carry had lost that word reached 3.96 of the allowed 4
    yardsticks in k_composite_c there).  On ``carry_rows`` the carried number is one fp32 value the
    test can compute from the device's own weight of the absorbing sample, so the opaque sample's
    weight must equal it exactly: through the scan, the lane-63 readlane of both halves and every
    later chunk, in k_composite_c<1..4> and k_composite alike."""
    rays, z, raw, a, b = ms.carry_rows(K, K)
    w = abi_composite(rays, z, raw, False)[0].cpu()
    rows = torch.arange(ms.N_ROWS)
    w_a, w_b = w[rows, a], w[rows, b]
    alpha64 = 1 - torch.exp(-(z[rows, a + 1] - z[rows, a]).double() * raw[rows, a, 3].double())
    # sigma delta <= 1.7 rounded to fp32, an expf of 1 ulp and the rounding of 1 - e: under 3 x 2^-24
    assert bool(((w_a.double() - alpha64).abs() <= 4 * 2.0 ** -24).all()), (w_a, alpha64)
    assert bool((w_a > 0.09).all()) and bool((w_a < 0.9).all())
    assert torch.equal(w_b, ms.carried_weight(w_a)), (K, (w_b - ms.carried_weight(w_a)).tolist())
    rest = w.clone()
    rest[rows, a] = 0.0
    rest[rows, b] = 0.0
    assert float(rest.abs().max()) == 0.0


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
@pytest.mark.parametrize("K", ms.POISON_KS)
def test_composite_nonfinite_sigma_stays_in_its_ray(K, poison):
    """A NaN sigma (max_nc keeps it a NaN, as torch.relu does) or a +inf sigma on a sample with a
    non-zero delta, in ray 2 and then in ray 3: the two rays one wave of k_composite_c marches.
    Every other ray keeps the bits of the clean run; in the poisoned ray the weights before the
    sample keep them too, what the fp64 reference makes non-finite is non-finite, and what it keeps
    finite matches it.  The sample, K / 2 - 3, lies in chunk 0 for K = 128 (before the opaque
    samples 63 / 64: the NaN reaches chunk 1 through the carry) and behind them for K = 256, 300."""
    cases, pooled = composite_reference()
    rays, z, raw, _ = cases[(K, True)]
    clean = [t.cpu() for t in abi_composite(rays, z, raw, True)]
    p = K // 2 - 3
    for ray in (2, 3):
        bad = raw.clone()
        bad[ray, p, 3] = poison
        assert float(z[ray, p + 1] - z[ray, p]) > 0.0
        r64 = ms.composite_ref64(rays, z, bad, True)
        got = [t.cpu() for t in abi_composite(rays, z, bad, True)]
        others = [b for b in range(ms.N_ROWS) if b != ray]
        for name, a, c in zip(NAMES, got, clean):
            assert torch.equal(a[others], c[others]), (name, ray)
        assert torch.equal(got[0][ray, :p], clean[0][ray, :p])
        where = {}
        for name, a, b in zip(NAMES, got, r64):
            assert not bool(torch.isfinite(a[~torch.isfinite(b)]).any()), (name, ray)
            where[name] = torch.isfinite(b)
        if poison != poison:
            assert not bool(torch.isfinite(r64[0][ray, p:]).any()) and not bool(torch.isfinite(r64[2][ray]))
        else:
            assert bool(torch.isfinite(r64[0]).all())
        check_composite("K=%d ray %d sigma %s" % (K, ray, poison), got, r64, pooled, where)


# ----------------------------------------------------------------- sampler --
def hip_sample_fine(c, **over):
    c = dict(c, **over)
    return ops.sample_fine(c["rays"].to(DEV), c["zc"].to(DEV), c["w"].to(DEV), c["depth"].to(DEV), c["kf"],
                           c["kfd"], ms.DEPTH_STD, c["u"].to(DEV), c["uj"].to(DEV), c["nd"].to(DEV),
                           c["lindisp"]).cpu()


@pytest.mark.parametrize("kc,kf,kfd,lindisp", ms.SAMPLER_CASES)
def test_sample_fine_peaked_pdf(kc, kf, kfd, lindisp):
    """``pnr_sample_fine`` on spike, split, all-zero and composite-made weight rows with draws
    placed in the heaviest bins (``placed_draws``), coarse depths of exactly near, exactly far and
    far + 1 (every depth sample clamps onto one value) and a ray with near == far: flat cdfs with
    one step across the cdf carry chunks, and sorts full of equal and near-equal keys."""
    c = ms.sampler_inputs(kc, kf, kfd, lindisp)
    ref = ms.sampler_ref(c)
    zf = hip_sample_fine(c)
    assert zf.shape == ref.shape and bool(torch.isfinite(zf).all())
    assert_close(zf, ref, "z_fine (%d, %d, %d)" % (kc, kf, kfd), 2e-6, 2e-6)
    assert bool((zf[:, 1:] >= zf[:, :-1]).all())
    for b in range(zf.shape[0]):
        assert bool(torch.isin(c["zc"][b], zf[b]).all()), b   # the sort moves values, it makes none


@pytest.mark.parametrize("kc,kf,kfd,lindisp", ms.SAMPLER_POISON_CASES)
def test_sample_fine_nonfinite_ray_stays_in_its_ray(kc, kf, kfd, lindisp):
    """One ray at a time gets a NaN weight, an inf coarse depth or a NaN coarse depth estimate;
    every other ray's z_fine keeps the bits of the clean run.  What the poisoned ray itself
    returns is printed, not asserted (fminf / fmaxf in the sort and the clamp drop NaNs; changing
    that is not this test's business).  Observed on an MI355X, the same in both cases and on the
    first, a middle and the last ray: a NaN weight makes the whole cdf NaN, every draw takes bin 0
    and the row comes back finite and sorted; an inf coarse depth comes back as one inf in the last
    place behind the sorted finite values; a NaN depth estimate is dropped by the clamp, all kfd
    depth samples come back as ``far``, and the row has no NaN."""
    c = ms.sampler_inputs(kc, kf, kfd, lindisp)
    clean = hip_sample_fine(c)
    B = clean.shape[0]
    for ray in (0, B // 2, B - 1):
        others = [b for b in range(B) if b != ray]
        for kind in ("nan weight", "inf z_coarse", "nan depth"):
            t = {"nan weight": "w", "inf z_coarse": "zc", "nan depth": "depth"}[kind]
            bad = c[t].clone()
            if t == "depth":
                bad[ray] = float("nan")
            else:
                bad[ray, kc // 3] = float("inf") if t == "zc" else float("nan")
            zf = hip_sample_fine(c, **{t: bad})
            row = zf[ray]
            fin = row[torch.isfinite(row)]
            print("(%d, %d, %d) ray %d %s: %d NaN, %d inf, %d of %d values equal to the clean run, finite part "
                  "sorted %s" % (kc, kf, kfd, ray, kind, int(torch.isnan(row).sum()), int(torch.isinf(row).sum()),
                                 int((row == clean[ray]).sum()), row.numel(),
                                 bool((fin[1:] >= fin[:-1]).all())))
            assert torch.equal(zf[others], clean[others]), (ray, kind)


# ------------------------------------------------------------------ render --
N_RAYS = 256
# (kc, kf, kfd, lindisp, depth_std); lindisp comes with per-ray near / far
MARCH_CASES = [
    (64, 64, 0, False, 0.01),     # both passes fused, mode 3's single launch
    (64, 32, 16, False, 0.01),    # shipped conf: fine pass K = 96 separate
    (64, 64, 16, True, 0.01),     # lindisp + depth samples, per-ray near / far
    (128, 0, 0, False, 0.01),     # coarse only, two tiles per ray
    (32, 32, 0, False, 0.01),     # coarse K = 32 separate, fine K = 64 fused
    (64, 32, 16, False, 0.5),     # depth samples spread over the ray and clamp onto near / far
]
MARCH_PRECS = ["fp32", "f16x3", "f16"]


@functools.lru_cache(maxsize=None)
def surface_scene(n_rays, pick):
    return synth.scene_srn(seed=5, n_rays=n_rays, pick=pick)


def surface_net(sc, precision, fine="own"):
    """The surface model on the device; ``fine``: "own" MLP, "none" (mlp_fine = None), or "copy" (a
    deep copy of the coarse MLP)."""
    net = PixelNeRFNet(model_conf())
    net.mlp_precision = precision
    net.load_state_dict(ms.surface_state(synth.pixelnerf_state(1)), strict=False)
    if fine == "none":
        net.mlp_fine = None
    elif fine == "copy":
        net.mlp_fine = copy.deepcopy(net.mlp_coarse)
    net = net.to(DEV).eval()
    net.encode_latent(sc["latent"].to(DEV), sc["poses"].to(DEV), sc["focal"].to(DEV), (128, 128))
    return net


def march_rays(lindisp):
    rays = surface_scene(N_RAYS, "all")["rays"]
    if lindisp:   # as test_fused_march_matches_unfused: the fused epilogue reads near / far per ray
        rays = rays.clone()
        h = torch.from_numpy(synth.hash_uniform(17, N_RAYS).astype("float32"))
        rays[:, 6] = 0.2 + 0.6 * h
        rays[:, 7] = 2.5 + 1.5 * h
    return rays


@functools.lru_cache(maxsize=None)
def march_outputs(case, precision):
    """Renders of one case in every march mode, on the CPU: {(mode, return_z): {pass: {key: tensor}}}
    for modes 0 .. 3 with z and modes 1 .. 3 without, and the rays and streams they used."""
    kc, kf, kfd, lindisp, depth_std = case
    rays = march_rays(lindisp)
    streams = synth.rng_streams(6, N_RAYS, kc, kf, kfd)
    net = surface_net(surface_scene(N_RAYS, "all"), precision)
    r = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, depth_std=depth_std, white_bkgd=True,
                     lindisp=lindisp)
    outs = {}
    for mode, return_z in [(0, True), (1, True), (2, True), (3, True), (1, False), (2, False), (3, False)]:
        r.march_mode, r.return_z, r.streams = mode, return_z, streams
        with torch.no_grad():
            o = r(net, rays[None].to(DEV), want_weights=True)
        torch.cuda.synchronize()
        outs[(mode, return_z)] = {p: {k: o[p][k].cpu() for k in ("rgb", "depth", "weights", "z") if k in o[p]}
                                  for p in (("coarse", "fine") if kf > 0 else ("coarse",))}
    return outs, rays, streams


@pytest.mark.parametrize("precision", MARCH_PRECS)
@pytest.mark.parametrize("case", MARCH_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_march_modes_bit_identical_on_a_surface(case, precision):
    """Modes 1, 2 and 3 against the separate kernels (mode 0) on a model that puts an opaque
    surface on every ray: rgb, depth, weights and z of both passes, with and without return_z."""
    outs, _, _ = march_outputs(case, precision)
    base = outs[(0, True)]
    w = base["coarse"]["weights"][0]
    print("%s %s: mean largest coarse weight %.4f, samples with w > 1e-3 per ray %.2f" % (
        case, precision, float(w.max(-1)[0].mean()), float((w > 1e-3).sum(-1).float().mean())))
    for (mode, return_z), o in outs.items():
        for p, ref in base.items():
            assert ("z" in o[p]) == return_z
            for k in ("rgb", "depth", "weights") + (("z",) if return_z else ()):
                assert torch.equal(o[p][k], ref[k]), (mode, return_z, p, k, float((o[p][k] - ref[k]).abs().max()))


@pytest.mark.parametrize("precision", MARCH_PRECS)
@pytest.mark.parametrize("case", MARCH_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_fine_samples_follow_the_device_coarse_pass(case, precision):
    """Mode 2's z_fine of every ray is what the reference algorithm draws from the device's own
    coarse depths, weights and depth estimate with the injected streams (or its alternative for
    a draw within parity.MARGIN of a cdf entry, and then the ray has such a draw), and each
    pass's composite is consistent with the weights and depths it returns.  (No end-to-end
    comparison with the oracle's MLP: the scaled sigma head multiplies the MLP's admitted fp32
    error by 1000; the composite and sampler tests above tie each stage to the oracle.)"""
    kc, kf, kfd, lindisp, depth_std = case
    outs, rays, streams = march_outputs(case, precision)
    o = outs[(2, True)]
    if kf > 0:
        co = o["coarse"]
        zf = o["fine"]["z"][0]
        sets = parity.expected_fine_sets(rays, co["z"], co["weights"], co["depth"], streams, kc, kf, kfd,
                                         depth_std=depth_std, lindisp=lindisp)
        match = [parity.close_mask(zf, ze, 2e-6, 2e-6).all(-1) for ze in sets]
        alt_only = match[1] & ~match[0]
        print("%s %s: %d of %d rays match only the marginal alternative" % (case, precision, int(alt_only.sum()), N_RAYS))
        assert bool((match[0] | match[1]).all()), torch.nonzero(~(match[0] | match[1])).reshape(-1).tolist()
        if kf - kfd > 0 and bool(alt_only.any()):
            dist = parity.boundary_distance(co["weights"][0], streams[1])
            assert bool((dist[alt_only] <= parity.MARGIN).all()), dist[alt_only]
    for p, t in o.items():
        w, z = t["weights"][0].double(), t["z"][0].double()
        K = w.shape[-1]
        sw = w.sum(-1)
        assert bool((w >= 0).all()) and float(sw.max()) <= 1.0 + 1e-5, (p, float(sw.max()))
        err = (t["depth"][0].double() - (w * z).sum(-1)).abs()
        assert bool((err <= K * 2.0 ** -24 * (w * z).abs().sum(-1)).all()), (p, float(err.max()))
        rgb = t["rgb"][0].double()
        assert bool((rgb >= (1.0 - sw - 1e-6).unsqueeze(-1)).all()) and bool((rgb <= 1.0 + 1e-6).all()), p


def test_fine_pass_reuses_coarse_outputs_on_a_surface():
    """mlp_fine = None against a deep copy of the coarse MLP, 64 + 128 samples of which 16 depth
    samples with depth_std 0.5, on the surface model: the merge of the coarse pass's outputs into
    the sorted fine samples (k_merge_raw behind the index-carrying LDS sort) meets clusters of
    near-equal depths and clamped ties.  rgb, depth and weights of both passes are bitwise equal."""
    sc = surface_scene(96, "hash")
    streams = synth.rng_streams(6, 96, 64, 128, 16)
    outs = []
    for fine in ("none", "copy"):
        r = NeRFRenderer(n_coarse=64, n_fine=128, n_fine_depth=16, depth_std=0.5, white_bkgd=True)
        r.streams = streams
        r.return_z = True
        with torch.no_grad():
            outs.append(r(surface_net(sc, "f16x3", fine), sc["rays"][None].to(DEV), want_weights=True))
    torch.cuda.synchronize()
    w = outs[0].coarse.weights[0]
    print("reuse: min sum w %.6f, mean largest coarse weight %.4f" % (float(w.sum(-1).min()), float(w.max(-1)[0].mean())))
    assert float(w.max(-1)[0].mean()) > 0.9
    for part in ("coarse", "fine"):
        for k in ("rgb", "depth", "weights", "z"):
            assert torch.equal(outs[0][part][k], outs[1][part][k]), (part, k)
