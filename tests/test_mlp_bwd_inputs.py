"""The inputs of tests/test_gpu_mlp_bwd_inputs.py are what they claim to be (CPU only).

tests/mlp_bwd_inputs.py builds ``d_o`` shaped like a trained scene's, reads and rearranges the
activation save, and states the per-point bound.  Checked here for every case the GPU file uses:
the builders' conditions, the mask decoder against an encoder written from the header text alone,
the point permutation's round trip, and that the yardsticks (``train.mlp_backward`` in fp64 and in
fp32) are finite on these inputs with the fp32 one inside the bound: the GPU test's escape (4 x the
fp32 backward's own per-point error) then widens the bound by at most 4.
"""
import copy

import numpy as np
import pytest
import torch

import mlp_bwd_inputs as mb
from pnr import synth
from pnr.models import PixelNeRFNet

NOMINAL_CU = 256
ALL_P = sorted({s[0] for s in mb.SHAPES.values()} | {e[0] for e in mb.EDGES} | set(mb.uneven_counts(NOMINAL_CU)))


def mlp_of(n_blocks, combine_layer, seed=11):
    mlp = dict(type="resnet", n_blocks=n_blocks, d_hidden=512, combine_layer=combine_layer, combine_type="average")
    conf = dict(use_encoder=True, use_xyz=True, use_code=True, code=dict(num_freqs=6, freq_factor=1.5,
                                                                         include_input=True),
                use_viewdirs=True, use_code_viewdirs=False, mlp_coarse=dict(mlp), mlp_fine=dict(mlp),
                encoder=dict(backbone="resnet34", pretrained=False, num_layers=4))
    net = PixelNeRFNet(conf)
    net.load_state_dict(synth.pixelnerf_state(seed, n_blocks=n_blocks, combine_layer=combine_layer), strict=False)
    return net.mlp_coarse


@pytest.mark.parametrize("P", [s[0] for s in mb.SHAPES.values()])
@pytest.mark.parametrize("name", mb.BUILDERS)
def test_builders_meet_their_conditions(name, P):
    d = mb.build(name, P, 5)            # every builder asserts its own conditions
    assert d.shape == (P, 4) and d.dtype == torch.float32 and bool(torch.isfinite(d).all())
    assert torch.equal(d, mb.build(name, P, 5))
    a = d.abs().amax(1)
    if name in ("surface", "zero_tile", "sigma_only", "rgb_only"):
        tiny = torch.finfo(torch.float32).tiny
        assert int((a == 0).sum()) * 4 >= P
        assert mb._tiles_all_zero(d)
        assert bool(((d.abs() > 0) & (d.abs() < tiny)).any())
        assert int((a >= 2.0 ** -3).sum()) * 100 >= P
        # zeros behind the surface: in every ray with a surface the last nonzero point is an O(1) one
        for r in range(0, P, mb.K_RAY):
            ray = a[r:r + mb.K_RAY]
            nz = torch.nonzero(ray).reshape(-1)
            if len(nz) > 1:
                assert float(ray[nz[-1]]) >= 0.125, (name, r)
    if name == "zero_tile":
        assert bool((d[64:128] == 0).all()) and int((d[128:192] != 0).any(1).sum()) == 1
    if name == "sigma_only":
        assert bool((d[:, :3] == 0).all())
    if name == "rgb_only":
        assert bool((d[:, 3] == 0).all())
    if name == "wide":
        e = set(np.frexp(a.double().numpy())[1].tolist())
        assert len(e) >= 50 and float(a.min()) >= 2.0 ** -62 and float(a.max()) <= 1.0
    if name == "big":
        assert float(a.max()) >= 2.0 ** 59 and float(a.max()) <= 2.0 ** 60 and float(a.min()) >= 0.25


@pytest.mark.parametrize("P", ALL_P)
def test_wide_at_every_point_count(P):
    d = mb.wide(P, P)
    assert d.shape == (P, 4) and bool((d != 0).all())


@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("P", [s[0] for s in mb.SHAPES.values()])
def test_poison_point_is_inside_its_tile(kind, P):
    d, p = mb.poison(kind, P, 9)
    bad = ~torch.isfinite(d).all(1)
    assert torch.nonzero(bad).reshape(-1).tolist() == [p]
    assert p % 64 not in (0, 63) and p != P - 1
    assert bool(torch.isnan(d[p]).all()) if kind == "nan" else bool((d[p] == float("inf")).all())
    clean = mb.wide(P, 9)
    keep = torch.arange(P) != p
    assert torch.equal(d[keep], clean[keep])


def header_encode(bits):
    """The mask bytes of one row from include/pnr_abi.h's sentence alone: [activation n > 0] of
    n = 64 w + 16 r + 4 g + e (w, r, g, e = 0..7, 0..3, 0..3, 0..3) at bit 4 (r & 1) + e of byte
    8 w + 2 g + (r >> 1)."""
    out = [0] * 64
    for w in range(8):
        for r in range(4):
            for g in range(4):
                for e in range(4):
                    if bits[64 * w + 16 * r + 4 * g + e]:
                        out[8 * w + 2 * g + (r >> 1)] |= 1 << (4 * (r & 1) + e)
    return out


def test_decode_masks_matches_the_header_text():
    g = torch.Generator().manual_seed(3)
    bits = torch.rand(9, 512, generator=g) < 0.4
    bits[0], bits[1] = False, True
    bits[2] = torch.arange(512) == 77
    enc = torch.tensor([header_encode(row.tolist()) for row in bits], dtype=torch.uint8)
    assert torch.equal(mb.decode_masks(enc), bits)
    assert torch.equal(mb.encode_masks(bits), enc)
    # every (byte, bit) is used exactly once
    one = torch.zeros(512, 64, dtype=torch.uint8)
    for n in range(512):
        row = [False] * 512
        row[n] = True
        one[n] = torch.tensor(header_encode(row), dtype=torch.uint8)
    assert int(mb.decode_masks(one).sum()) == 512 and torch.equal(mb.decode_masks(one), torch.eye(512).bool())


@pytest.mark.parametrize("P,ns,nb", [(200, 1, 5), (136, 2, 2), (65, 3, 8), (1, 3, 2)])
def test_save_regions_and_permutation_round_trip(P, ns, nb):
    save = mb.synthetic_save(P, nb, ns, seed=P)
    n = mb.save_floats(P, nb, ns)
    assert save.numel() == n
    r = mb.save_regions(save, P, nb, ns)
    R = ns * P
    assert r["feat"].shape == (R, 64) and r["z"].shape == (R, 512)
    assert len(r["relu"]) == len(r["mask"]) == 2 * nb + 1
    # the regions tile the save exactly, in the header's order
    ptrs = [r["feat"], r["z"]] + r["relu"] + r["mask"]
    off = save.data_ptr()
    for t in ptrs:
        assert t.data_ptr() == off
        off += t.numel() * t.element_size()
    assert off == save.data_ptr() + 4 * n
    for x, m in zip(r["relu"], r["mask"]):
        assert m.shape == (R, 64) and m.dtype == torch.uint8
        assert torch.equal(mb.decode_masks(m), x > 0)
    perm = mb.hashed_perm(P, 31)
    moved = mb.permute_points(save, perm, P, nb, ns)
    rm = mb.save_regions(moved, P, nb, ns)
    for v in range(ns):
        assert torch.equal(rm["z"][v * P + perm], r["z"][v * P: (v + 1) * P])
        assert torch.equal(rm["mask"][nb][v * P + perm], r["mask"][nb][v * P: (v + 1) * P])
    if P > 2:
        assert not mb.same_bits(moved, save)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(P)
    assert mb.same_bits(mb.permute_points(moved, inv, P, nb, ns), save)
    # gather_points: a larger save tiled from the small one's rows
    src = torch.arange(2 * P + 3) % P
    tiled = mb.save_regions(mb.gather_points(save, src, P, nb, ns), 2 * P + 3, nb, ns)
    for v in range(ns):
        assert torch.equal(tiled["relu"][0][v * (2 * P + 3) + P: v * (2 * P + 3) + 2 * P], r["relu"][0][v * P: (v + 1) * P])


def yardstick_cases():
    out = []
    for key, (P, ns, nb, comb) in mb.SHAPES.items():
        out += [pytest.param(P, ns, nb, comb, name, id="%s-%s" % (key, name)) for name in mb.BUILDERS + ("nan", "inf")]
    out += [pytest.param(P, ns, nb, comb, "wide", id="edge-%d-%d-%d-%d" % (P, ns, nb, comb)) for P, ns, nb, comb in mb.EDGES]
    return out


@pytest.mark.parametrize("P,ns,nb,comb,name", yardstick_cases())
def test_yardsticks_are_finite_and_fp32_is_inside_the_bound(P, ns, nb, comb, name):
    """train.mlp_backward in fp64 and fp32 on a synthetic save, for every (shape, input) of the GPU
    module (the poisoned inputs with their point zeroed: the run the GPU test compares with); the
    device-dependent point counts of the GPU module use the same builder at other sizes."""
    torch.set_num_threads(8)
    mlp = mlp_of(nb, comb)
    save = mb.synthetic_save(P, nb, ns, seed=7)
    if name in ("nan", "inf"):
        d_o, p = mb.poison(name, P, 5)
        d_o[p] = 0.0
    else:
        d_o = mb.build(name, P, 5)
    _, r32 = mb.reference(mlp, save, d_o, P, ns)
    _, r64 = mb.reference(copy.deepcopy(mlp).double(), save.double(), d_o.double(), P, ns)
    nc = mb.stages(nb, comb, ns)[1]
    for i, t in enumerate(r64["dy"]):
        assert t.shape == (mb.dy_rows(i, P, nb, nc, ns), 512), (i, t.shape)
    sc = mb.s_clamp(mlp)
    assert (r64["d_zlat"] is None) == (min(comb, nb) == 0)
    zero = (d_o == 0).all(1)
    for k, (err, s) in mb.point_errors(r32, r64, P).items():
        assert bool(torch.isfinite(err).all()) and bool(torch.isfinite(s).all()), k
        bound = mb.TOL * torch.clamp(s, min=sc[k])
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
        # a zero d_o row gives an exactly zero reference
        assert bool((s[zero] == 0).all()), k
        if name in ("wide", "big"):
            assert bool((s > 0).all()), k
