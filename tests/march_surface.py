"""Surface-like inputs for the along-ray kernels: opaque samples, peaked pdfs, clustered draws.

A trained pixelNeRF puts one or two opaque samples on a ray (sigma 1e2 .. 1e4, alpha exactly 1,
transmittance 1e-10 and below), so the cdf of the fine sampler is flat with one step, nearly every
fine draw lands in the same one or two bins and the sorted fine depths are clusters 1e-6 apart.
The builders here make such inputs from seeds; tests/test_march_surface_inputs.py (CPU) keeps them
from becoming "nice" again and tests/test_gpu_march_surface.py feeds them to the kernels.  The case
lists of both files live here so that the CPU test checks exactly what the GPU test uses.
"""
import torch

from oracle import ref_cpu

NEAR, FAR = 0.3, 4.0
N_ROWS = 9

# (a) composite forward: S = 1 .. 4 of k_composite_c at both ends of its range, then the generic kernel
COMPOSITE_KS = [1, 2, 24, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 511, 1024]
# (b) non-finite sigma: one K per kernel family, the pair kernel at two S
POISON_KS = [64, 128, 256, 300]
# (c) pnr_sample_fine: (kc, kf, kfd, lindisp)
SAMPLER_CASES = [
    (64, 64, 0, False),      # register sort of 128, one cdf chunk
    (64, 32, 16, True),      # register sort with padding, depth samples, lindisp
    (129, 127, 0, False),    # LDS sort of 256 exactly filled, one cdf entry in the third chunk
    (300, 212, 20, True),    # LDS sort of 512, a partial fifth cdf chunk, lindisp
    (64, 960, 64, False),    # 14 rounds of draws per lane, 64 depth samples
    (960, 64, 0, False),     # 15 cdf chunks
    (1, 63, 0, False),       # a single bin
]
# (d) non-finite rays in the sampler: the register sort and the LDS sort, both with depth samples
SAMPLER_POISON_CASES = [(64, 32, 16, False), (300, 212, 20, True)]
DEPTH_STD = 0.01


def _background(K, seed):
    """9 rays with near 0.3 / far 4.0, jittered-stratified depths in between (every delta >= 0.2 of
    a stratum, 7e-4 at K = 1024), rgb U(0, 1) and a negative sigma everywhere (relu -> 0)."""
    g = torch.Generator().manual_seed(seed)
    B = N_ROWS
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), NEAR), torch.full((B, 1), FAR)], 1)
    lo, span = NEAR + 0.01 * (FAR - NEAR), 0.98 * (FAR - NEAR)
    t = (torch.arange(K, dtype=torch.float32) + 0.1 + 0.8 * torch.rand(B, K, generator=g)) / K
    z = torch.sort(lo + span * t, -1)[0]
    raw = torch.rand(B, K, 4, generator=g)
    raw[..., 3] = -(0.5 + torch.rand(B, K, generator=g))
    return rays, z, raw


def carry_rows(K, seed):
    """9 rays (K >= 2) whose transmittance is ONE fp32 number carried across the chunk boundaries:
    an absorbing sample a (sigma delta = 0.1 .. 1.7) and an opaque sample b > a (sigma 1e6: sigma
    delta >= 700, alpha exactly 1 under any expf), nothing else.  Before a the transmittance is 1,
    so w_a = alpha_a; between a and b it is the fp32 number fl(fl(1 - alpha_a) + 1e-10) held in a
    double, multiplied by ones; so w_b must be exactly that number, whatever expf returned for
    alpha_a.  a is spread over the ray; b is the last sample (its delta is far - z, the carry
    passes every later chunk) or a + 64 (one boundary).  Returns rays, z, raw, a (9,), b (9,)."""
    rays, z, raw = _background(K, seed)
    a = torch.tensor([(i * (K - 1)) // N_ROWS for i in range(N_ROWS)])
    b = torch.tensor([K - 1 if i % 2 == 0 else min(K - 1, int(a[i]) + 64) for i in range(N_ROWS)])
    rows = torch.arange(N_ROWS)
    delta_a = z[rows, a + 1] - z[rows, a]
    raw[rows, a, 3] = (0.1 + 0.2 * rows) / delta_a
    raw[rows, b, 3] = 1e6
    return rays, z, raw, a, b


def carried_weight(w_a):
    """The weight of ``carry_rows``' opaque sample from the weight of the absorbing one, in the
    reference's fp32 arithmetic (nerf.py:230, 1 - alphas + 1e-10)."""
    return 1 - w_a.float() + 1e-10


def composite_rows(K, seed):
    """9 rays (odd: the pair tail of k_composite_c and a partly filled block) of K samples:
    ``rays`` (9, 8), ``z`` (9, K) sorted in (0.3, 4.0), ``raw`` (9, K, 4).  z is jittered-stratified
    (every delta >= 0.2 of a stratum, so a sigma of 1e4 on a non-zero delta is opaque at every K
    used); the background sigma is negative (relu -> 0).  Sample indices are clamped into
    [0, K - 1], a later placement overwriting an earlier one that clamps onto the same sample.

    0  sigma 1e4 at sample 0
    1  sigma 1e4 at sample K - 1: its delta is far - z
    2  sigma 1e4 at sample 63, the last lane of a chunk
    3  sigma 1e4 at sample 64, the first lane of the next chunk
    4  a shell of sigma 1e1, 1e2, 1e3, 1e4 at samples 62 .. 65, across the chunk boundary
    5  sigma 1e4 everywhere: the transmittance runs through the whole double range down to zero
    6  sigma 30 at K / 3, then 1e4 at 2 K / 3
    7  five equal depths from K / 2 on with sigma 1e4 on them: zero deltas under a huge sigma
    8  near == far == z: every delta is zero"""
    rays, z, raw = _background(K, seed)

    def c(i):
        return min(max(i, 0), K - 1)

    raw[0, c(0), 3] = 1e4
    raw[1, K - 1, 3] = 1e4
    raw[2, c(63), 3] = 1e4
    raw[3, c(64), 3] = 1e4
    for sigma, i in ((1e1, 62), (1e2, 63), (1e3, 64), (1e4, 65)):
        raw[4, c(i), 3] = sigma
    raw[5, :, 3] = 1e4
    raw[6, c(K // 3), 3] = 30.0
    raw[6, c(2 * K // 3), 3] = 1e4
    h = K // 2
    z[7, h:h + 5] = z[7, h]
    raw[7, h:h + 5, 3] = 1e4
    rays[8, 6] = rays[8, 7] = 1.7
    z[8] = 1.7
    raw[8, :, 3] = 1e4
    return rays, z, raw


def composite_ref64(rays, z, raw, white):
    """``ref_cpu.composite`` evaluated in fp64 on the same (fp32-valued) inputs."""
    return ref_cpu.composite(rays.double(), z.double(), raw.double(), white)


def peaked_weights(kc, seed):
    """Coarse weight rows (B, kc) as a surface leaves them: a 1.0 spike in bin 0, in bin kc - 1, in
    bin 63 and in bin 64 (the last lane of a cdf chunk and the first of the next; when kc has
    them), a 0.97 / 0.03 split over two neighbouring bins, all zeros (uniform pdf), 1e-9 rand, and
    the nine weight rows ``ref_cpu.composite`` returns for ``composite_rows(kc, seed)``."""
    g = torch.Generator().manual_seed(seed)
    rows = []

    def spike(i, v=1.0):
        r = torch.zeros(kc)
        r[i] = v
        return r

    rows.append(spike(0))
    rows.append(spike(kc - 1))
    if kc > 63:
        rows.append(spike(63))
    if kc > 64:
        rows.append(spike(64))
    split = spike(kc // 2, 0.97)
    split[min(kc // 2 + 1, kc - 1)] += 0.03
    rows.append(split)
    rows.append(torch.zeros(kc))
    rows.append(1e-9 * torch.rand(kc, generator=g))
    w = ref_cpu.composite(*composite_rows(kc, seed), False)[0]
    return torch.cat([torch.stack(rows, 0), w], 0).contiguous()


def fine_cdf64(w):
    """The cdf of nerf.py:126-133 in fp64 from fp32 weights: (B, kc) -> (B, kc + 1)."""
    w = w.double() + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    return torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)


def placed_draws(w, nf, seed):
    """u (B, nf) fp32 placed by the fp64 cdf of ``w``: nf - nf // 2 of a ray's draws go into its two
    heaviest bins (three in the heaviest for one in the second), the rest into the other bins,
    always including bin 0 and bin kc - 1; the order of a ray's draws is shuffled.  A draw for bin i
    is cdf[i] + (0.25 + 0.5 r) (cdf[i + 1] - cdf[i]) with r in [0.25, 0.75), that is 0.375 .. 0.625
    of the bin, so searchsorted cannot depend on the cdf's rounding and no draw needs moving.  (r
    over all of [0, 1) would leave a quarter of the narrowest bin, 2.5e-6, which is only 6.4 times
    the fp32 cdf's distance from the fp64 one at kc = 300, 4.0e-7: the fp32 sum of the pdf's
    normaliser moves every entry behind a spike together.  test_march_surface_inputs.py asks 8.)"""
    g = torch.Generator().manual_seed(seed)
    B, kc = w.shape
    cdf = fine_cdf64(w)
    order = torch.sort(cdf[:, 1:] - cdf[:, :-1], dim=-1, descending=True, stable=True)[1]
    n_rest = nf // 2
    n_heavy = nf - n_rest
    second = order[:, min(1, kc - 1)]
    heavy = torch.where((torch.arange(n_heavy) % 4 == 3)[None, :], second[:, None], order[:, :1])
    flat = order[:, 2:] if kc > 2 else order
    pick = torch.randint(0, flat.shape[1], (B, n_rest), generator=g)
    rest = flat.gather(1, pick)
    if n_rest > 0:
        rest[:, 0] = 0
    if n_rest > 1:
        rest[:, 1] = kc - 1
    bins = torch.cat([heavy.expand(B, n_heavy), rest], 1)
    perm = torch.argsort(torch.rand(B, nf, generator=g), -1)
    bins = bins.gather(1, perm)
    r = 0.25 + 0.5 * torch.rand(B, nf, generator=g).double()
    lo, hi = cdf.gather(1, bins), cdf.gather(1, bins + 1)
    return (lo + (0.25 + 0.5 * r) * (hi - lo)).float().contiguous()


def sampler_inputs(kc, kf, kfd, lindisp, seed=None):
    """The inputs of one ``pnr_sample_fine`` case on ``peaked_weights``: rays (near 0.5, far 3.5;
    the last ray has near == far == 2.0), stratified coarse depths, placed draws, and coarse depths
    that include exactly near (ray 0), exactly far (ray 1) and far + 1 (ray 2: every depth sample
    clamps to far, a kfd-way tie)."""
    seed = 7 * kc + kf if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    w = peaked_weights(kc, seed)
    B = w.shape[0]
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), 0.5), torch.full((B, 1), 3.5)], 1)
    rays[B - 1, 6] = rays[B - 1, 7] = 2.0
    zc = ref_cpu.sample_coarse(rays, kc, torch.rand(B, kc, generator=g), lindisp)
    depth = 0.5 + 3.0 * torch.rand(B, generator=g)
    depth[0], depth[1], depth[2] = 0.5, 3.5, 4.5
    depth[B - 1] = 2.0
    nf = kf - kfd
    u = placed_draws(w, nf, seed + 1)
    uj = torch.rand(B, nf, generator=g)
    nd = torch.randn(B, kfd, generator=g)
    return dict(rays=rays, zc=zc, w=w, depth=depth, u=u, uj=uj, nd=nd, kc=kc, kf=kf, kfd=kfd, lindisp=lindisp)


def sampler_ref(c):
    """sort(cat(zc, ref_cpu.sample_fine, ref_cpu.sample_fine_depth)) of ``sampler_inputs``."""
    samps = [c["zc"], ref_cpu.sample_fine(c["rays"], c["w"], c["kc"], c["u"], c["uj"], c["lindisp"])]
    if c["kfd"] > 0:
        samps.append(ref_cpu.sample_fine_depth(c["rays"], c["depth"], c["kfd"], DEPTH_STD, c["nd"]))
    return torch.sort(torch.cat(samps, -1), -1)[0]


def surface_state(sd, scale=1000.0, thresh=0.2):
    """A copy of a ``synth.pixelnerf_state`` dict whose sigma head is a surface: in both MLPs
    lin_out.weight[3] is multiplied by ``scale`` and lin_out.bias[3] becomes scale (bias - thresh),
    so sigma = relu(scale (s - thresh)) of the original pre-activation s."""
    out = dict(sd)
    for p in ("mlp_coarse.", "mlp_fine."):
        if p + "lin_out.weight" not in sd:
            continue
        wt = sd[p + "lin_out.weight"].clone()
        b = sd[p + "lin_out.bias"].clone()
        wt[3] *= scale
        b[3] = scale * (b[3] - thresh)
        out[p + "lin_out.weight"], out[p + "lin_out.bias"] = wt, b
    return out
