"""Trained-scene-like inputs for the fused MLP backward (k_mlp_bwd, k_bias_reduce; CPU only).

The composite backward of an opaque surface hands ``pnr_mlp_backward*`` a ``d_o`` with exact zeros
behind the surface, values down to fp32 denormals in front of it, whole rays (whole 64-point
tiles) of zeros, a few O(1) points, and gradients in the sigma channel only or the rgb channels
only.  The kernel publishes every gradient image with a power-of-two scale PER POINT (per image
column: ``relu_colmax<false>`` / ``relu_store_split<false>``, ``scale_exp`` in mlp_layout.h), so
its accuracy is a per-point statement; the builders here make ``d_o`` that holds it to one.
tests/test_mlp_bwd_inputs.py (CPU) keeps the builders honest, tests/test_gpu_mlp_bwd_inputs.py
feeds them to the kernel.  The case lists of both files live here, so the CPU test checks what
the GPU test uses.

The bound (include/pnr_abi.h states it for ``pnr_mlp_backward*``).  For a point p and an output
tensor T (dy: every slot and view row of p; d_feat; d_zlat), s_p(T) = max |fp64 reference| over
p's rows of T, and every row of p is within TOL * max(s_p(T), s_clamp(T)) of fp64.

* TOL = 2e-5, the tolerance tests/test_gpu_train.py holds this kernel to per tensor.
* s_clamp: ``scale_exp`` gives a column with maximum m the exponent e = 14 - frexp_exp(m), so that
  m 2^e is in (2^13, 2^14], and clamps it to e <= 40: a column with m < 2^-26 keeps m 2^e below
  2^14 no longer by following m but by the clamp (from 2^-27 down it is stored with the fixed
  quantum 2^-64, the fp16 subnormal quantum 2^-24 over 2^40).  Every published column is a dy row
  of its point (dx and dh ARE the dy slots), so for dy the scale below which the exponent stops
  following the data is S_CLAMP_DY = 2^-26.  d_zlat and d_feat are images of such columns under
  lin_z and lin_in: |W^T v|_inf <= |W|_1 |v|_inf <= K A |v|_inf with K the layer's input width
  and A = 2^frexp_exp(max |W|) the power of two the weight pack scales the layer by
  (k_layer_escale), summed over the lin_z layers.  s_clamp(T) = 2^-26 * that factor.  Below it
  the bound is absolute, TOL * s_clamp(T).  (What a clamped column can actually lose is 2^-65 per
  element, 2^-65 |W|_1 per output: 2^-23 of that bound.)
* Upper end: ``scale_exp`` clamps at e >= -64, which keeps a column maximum up to 2^78 at or below
  2^14; ``big`` tests ``d_o`` up to 2^60.
"""
import numpy as np
import torch

from pnr import synth, train

TOL = 2e-5
S_CLAMP_DY = 2.0 ** -26
TILE = 64
K_RAY = 64        # samples per ray of ``surface``: a zero ray is a zero tile

# (P, NS, n_blocks, combine_layer) of the two main shapes: three tiles and one of 8 points; two
# tiles and one of 8 with the view rows v * 136 + p off the tile grid
SHAPES = {"p200": (200, 1, 5, 3), "p136": (136, 2, 2, 1)}
BUILDERS = ("surface", "zero_tile", "sigma_only", "rgb_only", "wide", "big")
# point-count edges: a single ragged tile, P = 1, P = 64 +- 1; the view mean at both ends of the
# descriptor range with NS = 3
EDGES = [(1, 1, 5, 3), (63, 1, 5, 3), (64, 1, 5, 3), (65, 1, 5, 3),
         (1, 3, 8, 7), (65, 3, 8, 7), (1, 3, 2, 0), (65, 3, 2, 0)]
# the mask cases: both shapes and P = 65 with three views
MASK_CASES = [SHAPES["p200"], SHAPES["p136"], (65, 3, 8, 7)]


def uneven_counts(cu):
    """Point counts on a device of ``cu`` compute units (k_mlp_bwd launches min(tiles, cu)
    workgroups): cu + 1 tiles with a ragged last one (2 tiles on one workgroup, 1 on the others),
    and 2 cu - 1 tiles plus one point (a workgroup's second tile is the one-point tile)."""
    return [TILE * (cu + 1) - 7, TILE * (2 * cu - 1) + 1]


# ---------------------------------------------------------------------------- d_o builders --
def _hash(seed, n):
    return synth.hash_uniform(seed, n).astype(np.float64)


def _directions(P, seed):
    """(P, 4) values of magnitude in [0.5, 1) with hashed signs: a row's direction."""
    u = _hash(seed, 8 * P).reshape(2, P, 4)
    return (0.5 + 0.5 * u[0]) * np.where(u[1] < 0.5, -1.0, 1.0)


def _tiles_all_zero(d_o):
    P = d_o.shape[0]
    z = (d_o == 0).all(1)
    return [t for t in range((P + TILE - 1) // TILE) if bool(z[t * TILE:(t + 1) * TILE].all())]


def _check_surface(d_o, what):
    P = d_o.shape[0]
    a = d_o.abs()
    zero = (a == 0).all(1)
    tiny = torch.finfo(torch.float32).tiny
    assert int(zero.sum()) * 4 >= P, "%s: %d of %d points are exactly zero" % (what, int(zero.sum()), P)
    assert _tiles_all_zero(d_o), "%s: no all-zero tile" % what
    assert bool(((a > 0) & (a < tiny)).any()), "%s: no denormal entry" % what
    big = int((a.amax(1) >= 2.0 ** -3).sum())
    assert big * 100 >= P, "%s: %d of %d points at or above 2^-3" % (what, big, P)


def _surface(P, seed):
    """The magnitudes of ``surface`` as float64 (P,): per ray of K_RAY samples 1 - 3 samples of
    0.25 .. 1 around a hashed surface index s, 2^-(7 .. 9) per sample of decay in front of it
    (the transmittance of a medium in front of an opaque sample falls geometrically towards the
    camera's side of the gradient), exact 0 behind it; rays 1, 5, 9, .. entirely zero."""
    n_rays = (P + K_RAY - 1) // K_RAY
    h = _hash(seed, 4 * n_rays).reshape(4, n_rays)
    mag = np.zeros(n_rays * K_RAY)
    for r in range(n_rays):
        if r % 4 == 1:
            continue
        k = min(K_RAY, P - r * K_RAY)           # the last ray may be ragged
        width = 1 + int(3 * h[1, r])
        lo = min(24, max(k - width, 0))          # far enough from the ray's start to decay into denormals
        s = lo + int(h[0, r] * max(k - width - lo + 1, 1))
        rate = 7.0 + 2.0 * h[2, r]
        i = np.arange(k)
        front = np.exp2(-rate * (s - i[:s]) - 2.0 * h[3, r])
        m = np.zeros(k)
        m[:s] = front
        m[s:s + width] = 0.25 + 0.75 * _hash(seed + 17 + r, width)
        mag[r * K_RAY:r * K_RAY + k] = m
    return mag[:P]


def surface(P, seed, check=True):
    """d_o (P, 4) fp32 of an opaque surface's composite backward (see ``_surface``)."""
    d = torch.from_numpy((_surface(P, seed)[:, None] * _directions(P, seed + 1)).astype(np.float32))
    if check:
        _check_surface(d, "surface")
    return d


def zero_tile(P, seed):
    """``surface`` with points 64 .. 127 all zero and tile 2 (points 128 ..) holding a single
    nonzero point, neither its first nor its last.  P > 130."""
    assert P > 2 * TILE + 2
    d = surface(P, seed, check=False)
    d[TILE:2 * TILE] = 0.0
    n2 = min(TILE, P - 2 * TILE)
    keep = 2 * TILE + 1 + int(_hash(seed + 3, 1)[0] * (n2 - 2))
    row = torch.from_numpy((0.5 * _directions(1, seed + 4)[0]).astype(np.float32))
    d[2 * TILE:2 * TILE + n2] = 0.0
    d[keep] = row
    _check_surface(d, "zero_tile")
    assert 1 in _tiles_all_zero(d) and int((d[2 * TILE:3 * TILE] != 0).any(1).sum()) == 1
    return d


def sigma_only(P, seed):
    """``surface`` with the gradient in the sigma channel (column 3) only."""
    d = surface(P, seed)
    d[:, :3] = 0.0
    assert bool((d[:, 3] != 0).any())
    return d


def rgb_only(P, seed):
    """``surface`` with the gradient in the rgb channels (columns 0 .. 2) only."""
    d = surface(P, seed)
    d[:, 3] = 0.0
    assert bool((d[:, :3] != 0).any())
    return d


def _exponents(P, seed):
    """k (P,) in 0 .. 60: every run of 61 points is a hashed permutation of the 61 exponents."""
    n = (P + 60) // 61
    k = np.concatenate([np.argsort(_hash(seed + 101 * j, 61), kind="stable") for j in range(n)])
    return k[:P]


def wide(P, seed):
    """d_o (P, 4): per-point magnitudes 2^-k, k hashed over 0 .. 60, both signs, no zeros."""
    k = _exponents(P, seed)
    d = torch.from_numpy((np.exp2(-k.astype(np.float64))[:, None] * _directions(P, seed + 1)).astype(np.float32))
    assert bool((d != 0).all()) and bool((d < 0).any() or P < 2) and bool((d > 0).any() or P < 2)
    assert len(set(k.tolist())) >= min(P, 50), "wide covers %d of 61 exponents" % len(set(k.tolist()))
    return d


def big(P, seed):
    """d_o (P, 4): per-point magnitudes 2^k, k hashed over 0 .. 60 (entries up to 2^60)."""
    k = _exponents(P, seed + 7)
    d = torch.from_numpy((np.exp2(k.astype(np.float64))[:, None] * _directions(P, seed + 1)).astype(np.float32))
    assert bool(torch.isfinite(d).all()) and float(d.abs().max()) <= 2.0 ** 60
    assert float(d.abs().max()) >= 2.0 ** 59 or P < 61
    return d


def poison(kind, P, seed):
    """``wide`` with one point's row NaN or +Inf; the point is neither first nor last of its
    tile.  Returns (d_o, point)."""
    assert P >= 3
    d = wide(P, seed)
    n_tiles = (P + TILE - 1) // TILE
    t = int(_hash(seed + 5, 1)[0] * n_tiles)
    n = min(TILE, P - t * TILE)
    if n < 3:
        t, n = t - 1, TILE
    p = t * TILE + 1 + int(_hash(seed + 6, 1)[0] * (n - 2))
    d[p] = {"nan": float("nan"), "inf": float("inf")}[kind]
    assert 0 < p % TILE < n - 1
    return d, p


def build(name, P, seed):
    return {"surface": surface, "zero_tile": zero_tile, "sigma_only": sigma_only, "rgb_only": rgb_only,
            "wide": wide, "big": big}[name](P, seed)


def hashed_perm(P, seed):
    """A hashed permutation of 0 .. P - 1 as an int64 tensor."""
    return torch.from_numpy(np.argsort(_hash(seed, P), kind="stable").astype(np.int64))


# ---------------------------------------------------------------------------- the save --
def stages(n_blocks, combine_layer, ns):
    """(nb, nc): nc = the blocks that run once per view row (all of them with one view)."""
    return n_blocks, (min(combine_layer, n_blocks) if ns > 1 else n_blocks)


def dy_rows(i, P, n_blocks, nc, ns):
    """Rows of dy slot i that the kernel writes: ns P view rows for the per-view stages (the blocks
    before combine_layer, lin_in), P for the per-point ones.  Slots: [b] fc_0 of block b, [nb]
    lin_in, [nb + 1 + b] fc_1 of block b."""
    if i == n_blocks:
        return ns * P
    b = i if i < n_blocks else i - n_blocks - 1
    return ns * P if b < nc else P


def relu_rows(i, P, n_blocks, nc, ns):
    """Rows of relu region (and mask region) i that the forward writes.  Regions: [b] relu(x_b),
    [nb + b] relu(h_b), [2 nb] relu(x) into lin_out."""
    if i == 2 * n_blocks:
        return P
    b = i if i < n_blocks else i - n_blocks
    return ns * P if b < nc else P


def save_floats(P, n_blocks, ns):
    """Floats of the activation save (pnr_point_save_floats) for P points and ns views."""
    return ns * P * (64 + 512 * (2 + 2 * n_blocks) + 16 * (2 * n_blocks + 1))


def save_regions(save, P, n_blocks, ns=1):
    """Views of every region of the activation save as include/pnr_abi.h lays it out, R = ns P
    rows each: ``feat`` (R, 64), ``z`` (R, 512), ``relu`` [2 nb + 1] of (R, 512) (relu(x_b) of every
    block, relu(h_b) of every block, relu(x) into lin_out) and, for an fp32 save, ``mask``
    [2 nb + 1] of (R, 64) uint8: the sign masks of the relu regions in the same order."""
    R = ns * P
    feat, z, slot = train._save_views(save, P, n_blocks, ns=ns)
    out = dict(feat=feat, z=z, relu=[slot(i) for i in range(2 * n_blocks + 1)])
    if save.dtype == torch.float32:
        off = R * (64 + 512 * (2 + 2 * n_blocks))
        m = save[off: off + 16 * R * (2 * n_blocks + 1)].view(torch.uint8)
        out["mask"] = [m[64 * R * i: 64 * R * (i + 1)].view(R, 64) for i in range(2 * n_blocks + 1)]
    return out


def _mask_index():
    """(byte, bit) of channel n = 64 w + 16 r + 4 g + e: bit 4 (r & 1) + e of byte 8 w + 2 g + (r >> 1)."""
    n = np.arange(512)
    w, r, g, e = n // 64, (n % 64) // 16, (n % 16) // 4, n % 4
    return torch.from_numpy(8 * w + 2 * g + (r >> 1)), torch.from_numpy(4 * (r & 1) + e)


def decode_masks(mask_region):
    """(R, 64) uint8 -> (R, 512) bool, [activation n > 0] in channel order."""
    byte, bit = _mask_index()
    byte, bit = byte.to(mask_region.device), bit.to(mask_region.device)
    return ((mask_region[:, byte].to(torch.int32) >> bit.to(torch.int32)) & 1).bool()


def encode_masks(bits):
    """``decode_masks``' inverse: (R, 512) bool -> (R, 64) uint8."""
    byte, bit = _mask_index()
    out = torch.zeros(bits.shape[0], 64, dtype=torch.int32, device=bits.device)
    out.index_add_(1, byte.to(bits.device), bits.to(torch.int32) << bit.to(device=bits.device, dtype=torch.int32))
    return out.to(torch.uint8)


def gather_points(save, src, P_src, n_blocks, ns=1):
    """A new save of P_dst = len(src) points whose point q is point src[q] of ``save``: row
    v * P_dst + q of every region (masks included) is row v * P_src + src[q]."""
    src = torch.as_tensor(src, dtype=torch.int64, device=save.device)
    P_dst = src.numel()
    out = torch.empty(save_floats(P_dst, n_blocks, ns), dtype=save.dtype, device=save.device)
    a, b = save_regions(save, P_src, n_blocks, ns), save_regions(out, P_dst, n_blocks, ns)
    rows = torch.cat([v * P_src + src for v in range(ns)])

    def pairs():
        yield a["feat"], b["feat"]
        yield a["z"], b["z"]
        for key in ("relu", "mask"):
            for x, y in zip(a.get(key, []), b.get(key, [])):
                yield x, y

    for x, y in pairs():
        y.copy_(x[rows])
    return out


def permute_points(save, perm, P, n_blocks, ns=1):
    """A new save with point p of every view moved to perm[p]: row v * P + perm[p] of every
    region is row v * P + p of ``save``."""
    perm = torch.as_tensor(perm, dtype=torch.int64, device=save.device)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(P, dtype=torch.int64, device=save.device)
    return gather_points(save, inv, P, n_blocks, ns)


def same_bits(a, b):
    """Bit-for-bit equality of two fp32 tensors (NaN payloads and the sign of zero included; a
    save's mask bytes read as floats may be NaN patterns)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def synthetic_save(P, n_blocks, ns, seed):
    """A save with random contents for the CPU checks: features and z N(0, 1), relu regions
    relu(N(0, 1) - 0.3) (about 40 % active; exact zeros where inactive), masks consistent with
    them."""
    g = torch.Generator().manual_seed(seed)
    save = torch.zeros(save_floats(P, n_blocks, ns), dtype=torch.float32)
    r = save_regions(save, P, n_blocks, ns)
    r["feat"].copy_(torch.randn(r["feat"].shape, generator=g))
    r["z"].copy_(torch.randn(r["z"].shape, generator=g))
    for x, m in zip(r["relu"], r["mask"]):
        x.copy_(torch.relu(torch.randn(x.shape, generator=g) - 0.3))
        m.copy_(encode_masks(x > 0))
    return save


# ---------------------------------------------------------------------------- the bound --
def weight_scale(w):
    """2^frexp_exp(max |w|): the power of two above the layer's largest weight, which the f16x3
    pack scales the layer by (scale_exp, k_layer_escale)."""
    return float(2.0 ** np.frexp(float(w.detach().abs().max()))[1])


def s_clamp(mlp):
    """{tensor: scale} below which the bound is absolute (the module docstring derives it)."""
    lin_z = list(getattr(mlp, "lin_z", []))
    return {"dy": S_CLAMP_DY,
            "d_feat": S_CLAMP_DY * mlp.lin_in.weight.shape[1] * weight_scale(mlp.lin_in.weight),
            "d_zlat": S_CLAMP_DY * sum(512 * weight_scale(lz.weight) for lz in lin_z)}


def per_point_max(t, P):
    """max |t| over the rows of each point: t (P or ns P, C), view-major rows -> (P,) float64."""
    return t.double().abs().reshape(-1, P, t.shape[-1]).amax(dim=(0, 2))


def per_point(tensors, P):
    """``per_point_max`` over a list of tensors (the dy slots)."""
    out = per_point_max(tensors[0], P)
    for t in tensors[1:]:
        out = torch.maximum(out, per_point_max(t, P))
    return out


def reference(mlp, save, d_o, P, ns):
    """``train.mlp_backward`` with its per-layer output gradients: (g, {"dy": [slots, cut to the
    rows each uses], "d_feat": .., "d_zlat": .. or None})."""
    slots = {}
    with torch.no_grad():
        g, d_feat, d_zlat = train.mlp_backward(mlp, save, d_o, P, ns, dy_slots=slots)
    nb = mlp.n_blocks
    return g, dict(dy=[slots[i] for i in range(2 * nb + 1)], d_feat=d_feat, d_zlat=d_zlat)


def as_lists(out):
    """{"dy": [..], "d_feat": t, "d_zlat": t or None} -> {name: [tensors]} without the absent ones."""
    return {k: (v if isinstance(v, list) else [v]) for k, v in out.items() if v is not None}


def point_errors(got, ref64, P):
    """{tensor: (err_p, s_p)}: per point, max |got - fp64| and max |fp64| over its rows."""
    a, b = as_lists(got), as_lists(ref64)
    assert set(a) == set(b), (set(a), set(b))
    out = {}
    for k in b:
        assert len(a[k]) == len(b[k])
        for x, y in zip(a[k], b[k]):
            assert x.shape == y.shape, (k, x.shape, y.shape)
        err = per_point([x.double() - y.double() for x, y in zip(a[k], b[k])], P)
        out[k] = (err, per_point(b[k], P))
    return out
