"""The surface-like inputs of tests/test_gpu_march_surface.py are what they claim to be (CPU only).

tests/march_surface.py builds opaque composite rows, peaked pdfs with placed draws and a model
whose sigma head is a surface.  The GPU tests compare tightly and exclude nothing, which only
works while the oracle itself is stable on these inputs and every draw keeps its distance from the
cdf entries; and they only test what they mean to while the inputs stay opaque and peaked.  Both
are checked here for every case the GPU file uses.
"""
import pytest
import torch

import march_surface as ms
from oracle import parity, ref_cpu
from pnr import synth


@pytest.mark.parametrize("K", ms.COMPOSITE_KS)
def test_composite_rows_are_opaque_and_the_oracle_is_finite(K):
    rays, z, raw = ms.composite_rows(K, K)
    assert z.shape == (ms.N_ROWS, K) and raw.shape == (ms.N_ROWS, K, 4)
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    assert bool((z[:8] > ms.NEAR).all()) and bool((z[:8] < ms.FAR).all())
    assert float(raw[:5, :, 3].min()) < 0.0 or K == 1     # the background sigma is negative
    for white in (False, True):
        for out in (ref_cpu.composite(rays, z, raw, white), ms.composite_ref64(rays, z, raw, white)):
            for t in out:
                assert bool(torch.isfinite(t).all())
            w = out[0]
            # every row 0-7 has a sigma of 1e4 on a non-zero delta at every K
            assert float(w[:8].sum(-1).min()) >= 0.99, (K, w[:8].sum(-1))
            assert float(w[8].abs().max()) == 0.0
    w = ref_cpu.composite(rays, z, raw, False)[0]
    # one sample carries the ray, except where the row is built otherwise (4: a shell; 5: all
    # opaque; 6: a sigma-30 sample first)
    assert float(w[[0, 1, 2, 3, 7]].max(-1)[0].min()) >= 0.99
    if K > 1:
        d = z[:, 1:] - z[:, :-1]
        h = K // 2
        assert float(d[7, h:min(h + 4, K - 1)].abs().max() if h < K - 1 else 0.0) == 0.0   # the tie of row 7
        assert float(d[8].abs().max()) == 0.0


@pytest.mark.parametrize("K", [K for K in ms.COMPOSITE_KS if K >= 2])
def test_carry_rows_pin_the_carried_transmittance(K):
    """The identity the GPU test asserts is the reference's own: in fp32 ``ref_cpu.composite`` the
    opaque sample's weight is exactly 1 - w_a + 1e-10, every other weight is exactly zero, and
    wherever K allows the two samples lie in different 64-sample chunks."""
    rays, z, raw, a, b = ms.carry_rows(K, K)
    rows = torch.arange(ms.N_ROWS)
    assert bool((b > a).all()) and bool((a >= 0).all()) and bool((b < K).all())
    if K > 64:
        assert bool(((b // 64) > (a // 64)).any())
        assert len(set((b // 64 - a // 64).tolist())) >= min(2, (K - 1) // 64)
    x_b = torch.where(b + 1 < K, z[rows, (b + 1).clamp_max(K - 1)], rays[:, 7]) - z[rows, b]
    assert float((x_b * raw[rows, b, 3]).min()) >= 100.0       # exp(-100) = 0 in fp32: alpha_b is exactly 1
    w = ref_cpu.composite(rays, z, raw, False)[0]
    w_a, w_b = w[rows, a], w[rows, b]
    assert bool((w_a > 0.09).all()) and bool((w_a < 0.9).all())
    assert torch.equal(w_b, ms.carried_weight(w_a))
    assert int((w != 0).sum()) == 2 * ms.N_ROWS
    # and the number is not one a broken low word would leave alone: its last three bits vary
    assert len(set((w_b.view(torch.int32) & 7).tolist())) >= 3


@pytest.mark.parametrize("kc,kf,kfd,lindisp", ms.SAMPLER_CASES + ms.SAMPLER_POISON_CASES)
def test_placed_draws_keep_their_distance_and_cluster(kc, kf, kfd, lindisp):
    c = ms.sampler_inputs(kc, kf, kfd, lindisp)
    w, u = c["w"], c["u"]
    B, nf = u.shape
    assert nf == kf - kfd and w.shape == (B, kc)
    assert bool((u >= 0).all()) and bool((u < 1).all())
    cdf64 = ms.fine_cdf64(w)
    cdf32 = parity.fine_cdf(w)
    assert bool((cdf64[:, 1:] > cdf64[:, :-1]).all())
    bins = torch.clamp(torch.searchsorted(cdf64, u.double().contiguous(), right=True) - 1, 0, kc - 1)
    assert torch.equal(bins, parity.fine_bins(w, u))
    lo, hi = cdf64.gather(1, bins), cdf64.gather(1, bins + 1)
    dist = torch.minimum(u.double() - lo, hi - u.double())
    assert bool((dist >= 0.2 * (hi - lo)).all()), float((dist / (hi - lo)).min())
    # the fp32 cdf the oracle and the device search, against the fp64 one the draws were placed by:
    # the largest rounding anywhere in the case, not only at a draw's own two entries
    cdf_err = float((cdf32.double() - cdf64).abs().max())
    print("(%d, %d, %d): narrowest bin %.3g, min draw distance %.3g, max |cdf32 - cdf64| %.3g, ratio %.1f" % (
        kc, kf, kfd, float((cdf64[:, 1:] - cdf64[:, :-1]).min()), float(dist.min()), cdf_err,
        float(dist.min()) / max(cdf_err, 1e-30)))
    assert float(dist.min()) >= 8.0 * cdf_err, (float(dist.min()), cdf_err)
    # clustered: at least half of a ray's draws in its two heaviest bins (bins as wide as the second
    # widest count: a uniform row has no heaviest bin); the flat bins include both ends
    width = cdf64[:, 1:] - cdf64[:, :-1]
    second = torch.topk(width, min(2, kc), -1)[0][:, -1:]
    in_top = width.gather(1, bins) >= second
    assert bool((in_top.sum(-1) * 2 >= nf).all())
    assert bool((bins == 0).any(-1).all()) and bool((bins == kc - 1).any(-1).all())
    # the depth samples tie: exactly near, exactly far, far + 1, and a ray with near == far
    rays, depth = c["rays"], c["depth"]
    assert float(depth[0]) == float(rays[0, 6]) and float(depth[1]) == float(rays[1, 7])
    assert float(depth[2]) == float(rays[2, 7]) + 1.0
    assert float(rays[B - 1, 6]) == float(rays[B - 1, 7])
    if kfd > 0:
        zd = ref_cpu.sample_fine_depth(rays, depth, kfd, ms.DEPTH_STD, c["nd"])
        assert bool((zd[2] == rays[2, 7]).all()) and bool((zd[B - 1] == rays[B - 1, 6]).all())
        assert bool((zd[0] == rays[0, 6]).any()) and bool((zd[1] == rays[1, 7]).any())
    ref = ms.sampler_ref(c)
    assert bool(torch.isfinite(ref).all())


def test_surface_model_makes_every_ray_opaque():
    """The CPU oracle render of the scaled sigma head: every ray hits a surface, and the coarse
    weight sits on about one sample (synth.pixelnerf_state alone: largest weight about 0.19)."""
    sd = ms.surface_state(synth.pixelnerf_state(1))
    base = synth.pixelnerf_state(1)
    for p in ("mlp_coarse.", "mlp_fine."):
        assert torch.equal(sd[p + "lin_out.weight"][:3], base[p + "lin_out.weight"][:3])
        assert torch.equal(sd[p + "lin_out.weight"][3], base[p + "lin_out.weight"][3] * 1000.0)
        assert torch.equal(sd[p + "lin_out.bias"][3], 1000.0 * (base[p + "lin_out.bias"][3] - 0.2))
        assert torch.equal(synth.pixelnerf_state(1)[p + "lin_out.bias"], base[p + "lin_out.bias"])
    sc = synth.scene_srn(seed=5, n_rays=32, pick="hash")
    streams = synth.rng_streams(6, 32, 64, 64, 0)
    scene = ref_cpu.Scene(sc["latent"], sc["poses"], sc["focal"], 128, 128, None)
    with torch.no_grad():
        ref = ref_cpu.render(lambda p, c, d: ref_cpu.pixelnerf_forward(sd, scene, p, c, d),
                             sc["rays"][None], 64, 64, 0, streams, True)
    wc, wf = ref["coarse"]["weights"][0], ref["fine"]["weights"][0]
    print("surface model: min sum w coarse %.6f fine %.6f, mean largest coarse weight %.4f, samples with "
          "w > 1e-3 per ray %.2f" % (float(wc.sum(-1).min()), float(wf.sum(-1).min()),
                                     float(wc.max(-1)[0].mean()), float((wc > 1e-3).sum(-1).float().mean())))
    assert bool((wc.sum(-1) > 0.99).all()) and bool((wf.sum(-1) > 0.99).all())
    assert float(wc.max(-1)[0].mean()) > 0.9
