"""The fused MLP backward held to a per-point bound on trained-scene gradients (``-m gpu``).

``pnr_mlp_backward_views`` (k_mlp_bwd, k_bias_reduce) publishes every gradient image with a
power-of-two scale per point, so its accuracy is a per-point statement; the per-tensor comparison
of tests/test_gpu_train.py cannot see a point with a 2^-20 gradient that is wrong by 100 %.  Here
the kernel runs on ``d_o`` shaped like an opaque surface's composite backward
(tests/mlp_bwd_inputs.py; tests/test_mlp_bwd_inputs.py keeps the builders honest on the CPU) and
every point is compared on its own.

The bound (tests/mlp_bwd_inputs.py derives it, include/pnr_abi.h states it).  For a point p and an
output tensor T (dy: every slot and view row of p; d_feat; d_zlat), s_p(T) = max |fp64| over p's
rows of T; the fp64 reference is ``train.mlp_backward`` on ``copy.deepcopy(mlp).double()`` and
``save.double()``, on the device.

(a) every row of p is within TOL max(s_p(T), s_clamp(T)) of fp64, TOL = 2e-5 (this kernel's
    tolerance in tests/test_gpu_train.py, per point instead of per tensor); s_clamp(dy) = 2^-26,
    the column maximum below which ``scale_exp``'s clamp e <= 40 and not the data sets the
    exponent; s_clamp(d_feat) = 2^-26 d_in A(lin_in), s_clamp(d_zlat) = 2^-26 sum 512 A(lin_z b),
    A = the power of two above the layer's largest weight (the pack's weight scale).  Only where
    a point exceeds that is the bound 4 x the fp32 torch backward's own error on that point
    against fp64 (both numbers are printed then).  A point whose fp64 reference is entirely zero
    is exactly zero in every output.  Parameter gradients (``mlp_backward_fused``, both
    ``wgrad_arith``) keep the per-tensor rule: max(2e-5 max |fp64|, 4 x the fp32 backward's error).
(b) position invariance, bitwise: a point's rows do not depend on where in the launch it sits.
(c) point-count edges (one ragged tile, P = 1, 64 +- 1, uneven tiles per workgroup) with
    ``d_bias`` checked on its own against the fp64 column sums of the kernel's dy (the fp32
    summation bound n 2^-24 sum |dy|), and bitwise repeatability.
(d) the saved relu sign masks equal ``relu region > 0``; an activation of exactly 0 passes no
    gradient.
(e) a NaN / Inf row of ``d_o`` stays in its point's rows.
(f) an in-place weight update re-packs W^T.

Measured on an MI355X (MEASURED lines of test_per_point_accuracy): the kernel's worst
err / bound over all points and the three tensors, and the fp32 torch backward's own worst
err / (TOL max(s_p, s_clamp)) on the same case.  No point needed the 4 x escape.
    builder      P = 200 (NS 1, 5 / 3)      P = 136 (NS 2, 2 / 1)
                 kernel   fp32 torch        kernel   fp32 torch
    surface      0.058    0.045             0.058    0.040
    zero_tile    0.058    0.045             0.033    0.037
    sigma_only   0.045    0.044             0.043    0.040
    rgb_only     0.037    0.048             0.037    0.048
    wide         0.050    0.059             0.047    0.057
    big          0.052    0.062             0.047    0.057
Parameter gradients: worst err / bound 0.035 (f16x3) and 0.035 (bf16x6).
"""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch

import mlp_bwd_inputs as mb
from pnr import _lib, train
from pnr.models import PixelNeRFNet
from test_gpu_train import case, conf

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = mb.TOL


# ------------------------------------------------------------------------------ running --
def _rays_k(P):
    """P = rays * K with the largest K <= 64."""
    K = max(k for k in range(1, 65) if P % k == 0)
    return P // K, K


def make_case(P, ns, n_blocks, comb, edit=None):
    """A model, its forward's activation save over P points and ns views (as
    tests/test_gpu_train.py makes them), and the sizes.  ``edit(mlp)`` changes the weights first."""
    n_rays, K = _rays_k(P)
    cs = case(sb=1, rays_per_obj=n_rays, kc=K, ns=ns, combine_layer=comb, n_blocks=n_blocks)
    net = PixelNeRFNet(conf(comb, n_blocks))
    net.load_state_dict(cs["sd"], strict=False)
    net = net.to(DEV)
    net.mlp_precision = "f16x3"
    if edit is not None:
        with torch.no_grad():
            edit(net.mlp_coarse)
    net.encode_latent(cs["latent"].to(DEV), cs["poses"].to(DEV), cs["focal"].to(DEV),
                      (cs["width"], cs["height"]), c=cs["c"].to(DEV), num_objs=1)
    rays = cs["rays"].to(DEV).reshape(-1, 8).contiguous()
    t = torch.linspace(0.0, 1.0, K, device=DEV) if K > 1 else torch.full((1,), 0.5, device=DEV)
    z = (rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * t).contiguous()
    c = SimpleNamespace(net=net, mlp=net.mlp_coarse, P=P, ns=ns, nb=n_blocks, nc=mb.stages(n_blocks, comb, ns)[1],
                        rays=rays, z=z)
    assert net.num_views_per_obj == ns
    c.save = forward_save(c)
    assert c.save.numel() == mb.save_floats(P, n_blocks, ns)
    return c


def forward_save(c):
    ctx = SimpleNamespace()
    ctx.save_for_backward = lambda *ts: setattr(ctx, "saved", ts)
    with torch.no_grad():
        train.RenderPoints.forward(ctx, c.net, True, c.rays, c.z, c.net.encoder.latent_cl,
                                   *train.mlp_params(c.mlp))
    return ctx.saved[3]


small_case = functools.lru_cache(maxsize=None)(make_case)


def chain(c, d_o, save=None, P=None):
    """One ``pnr_mlp_backward_views`` launch (as ``train.mlp_backward_fused`` makes it) on ``save``
    (default: the case's own) over P points: ({"dy": [each slot cut to the rows the kernel writes],
    "d_feat", "d_zlat"}, d_bias (2 nb + 1, 512))."""
    save = c.save if save is None else save
    P = c.P if P is None else P
    mlp, nb, ns = c.mlp, c.nb, c.ns
    desc, packed, packed_t = mlp.packed_t(c.net.code, "f16x3")
    R = ns * P
    d_o = d_o.to(DEV).contiguous()
    assert d_o.shape == (P, 4) and save.numel() == mb.save_floats(P, nb, ns)
    # outputs and workspace start as NaN: a row or a bias partial the kernel fails to write shows
    nan = float("nan")
    dy = torch.full((2 * nb + 1, R, 512), nan, dtype=torch.float32, device=DEV)
    dzl = torch.full((R, 512), nan, dtype=torch.float32, device=DEV) if len(mlp.lin_z) else None
    w_out = mlp.lin_out.weight.detach().float().contiguous()
    sums = torch.full((2 * nb + 1, 512), nan, dtype=torch.float32, device=DEV)
    lib = _lib.load()
    wsb = lib.pnr_mlp_backward_workspace_bytes(desc, P)
    ws = torch.full((max(wsb, 1),), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.check(lib.pnr_mlp_backward_views(desc, _lib.ptr(packed), _lib.ptr(packed_t), _lib.ptr(w_out),
                                          _lib.ptr(save), _lib.ptr(d_o), P, ns, _lib.ptr(dy), _lib.ptr(dzl),
                                          _lib.ptr(sums), _lib.ptr(ws), wsb, _lib.stream_of(d_o.device)),
               "pnr_mlp_backward_views")
    feat = mb.save_regions(save, P, nb, ns)["feat"]
    with torch.no_grad():
        d_feat = train._lin_in_backward(mlp, {}, dy[nb], feat, sums[nb])
    slots = [dy[i, :mb.dy_rows(i, P, nb, c.nc, ns)] for i in range(2 * nb + 1)]
    return dict(dy=slots, d_feat=d_feat, d_zlat=dzl), sums


def references(c, d_o, save=None, P=None):
    """(g32, out32, g64, out64) of ``train.mlp_backward`` in fp32 and fp64 on the device."""
    save = c.save if save is None else save
    P = c.P if P is None else P
    d_o = d_o.to(DEV)
    g32, r32 = mb.reference(c.mlp, save, d_o, P, c.ns)
    g64, r64 = mb.reference(copy.deepcopy(c.mlp).double(), save.double(), d_o.double(), P, c.ns)
    return g32, r32, g64, r64


# ----------------------------------------------------------------------------- checking --
def check_points(what, c, got, r32, r64, P=None):
    """Rule (a) on every point; returns (worst err / bound of the kernel, of the fp32 backward)."""
    P = c.P if P is None else P
    sc = mb.s_clamp(c.mlp)
    errs, own = mb.point_errors(got, r64, P), mb.point_errors(r32, r64, P)
    worst, worst32 = 0.0, 0.0
    zero = torch.ones(P, dtype=torch.bool, device=DEV)
    for k, (err, s) in errs.items():
        zero &= s == 0
    for k, (err, s) in errs.items():
        assert bool(torch.isfinite(s).all()), (what, k)
        tol = TOL * torch.clamp(s, min=sc[k])
        o = own[k][0]
        bound = torch.where(err <= tol, tol, torch.maximum(tol, 4.0 * o))
        ratio = err / bound
        r = float(ratio.max())
        over = torch.nonzero(err > tol).reshape(-1)
        for p in over[:8].tolist():
            print("%s %s point %d: |fused - fp64| %.3g, |fp32 torch backward - fp64| %.3g, s_p %.3g, "
                  "TOL max(s_p, s_clamp) %.3g" % (what, k, p, float(err[p]), float(o[p]), float(s[p]), float(tol[p])))
        worst = max(worst, r)
        worst32 = max(worst32, float((o / tol).max()))
        print("%s %s: worst err / bound %.3g (point %d); fp32 torch backward's own %.3g" % (
            what, k, r, int(ratio.argmax()), float((o / tol).max())))
        assert bool((err <= bound).all()), (what, k, r, int(ratio.argmax()))
        # a point whose fp64 reference is entirely zero is exactly zero
        assert bool((err[zero] == 0).all()), (what, k, "nonzero output at a point with a zero reference")
    return worst, worst32, int(zero.sum())


def check_params(what, c, d_o, g32, g64):
    """Parameter gradients through ``mlp_backward_fused``, both weight-gradient arithmetics: the
    per-tensor rule against fp64."""
    keys = list(g32)
    refs64 = list(g64.values())
    assert len(keys) == len(refs64) == len(train.mlp_params(c.mlp))
    for arith in ("f16x3", "bf16x6"):
        with torch.no_grad():
            g, _, _ = train.mlp_backward_fused(c.mlp, c.net.code, "f16x3", c.save, d_o.to(DEV), c.P, c.ns, arith)
        assert len(g) == len(keys)
        worst = 0.0
        for param, b64 in zip(keys, refs64):
            a, b32 = g[param].double(), g32[param].double()
            scale = float(b64.abs().max())
            err, own = float((a - b64).abs().max()), float((b32 - b64).abs().max())
            bound = max(TOL * scale, 4.0 * own)
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
            assert err <= bound, (what, arith, tuple(param.shape), err, own, scale)
        print("%s parameter gradients (%s): worst err / bound %.3g" % (what, arith, worst))


def rows_of(t, P, idx):
    """Rows of the points idx in a (P or ns P, C) tensor, view-major."""
    k = t.shape[0] // P
    return t[torch.cat([v * P + idx for v in range(k)])]


def assert_same_points(what, a, pa, ia, b, pb, ib):
    """Points ia of run a (over pa points) equal points ib of run b bit for bit, in every tensor."""
    la, lb = mb.as_lists(a), mb.as_lists(b)
    assert set(la) == set(lb)
    for k in la:
        for j, (x, y) in enumerate(zip(la[k], lb[k])):
            assert mb.same_bits(rows_of(x, pa, ia), rows_of(y, pb, ib)), (what, k, j)


def assert_same_run(what, a, b):
    la, lb = mb.as_lists(a), mb.as_lists(b)
    for k in la:
        for j, (x, y) in enumerate(zip(la[k], lb[k])):
            assert mb.same_bits(x, y), (what, k, j)


def check_bias(what, c, got, sums, P=None):
    """d_bias alone: each column against the fp64 sum of the kernel's own dy column, within the
    fp32 summation bound n_rows 2^-24 sum |dy|."""
    for i, t in enumerate(got["dy"]):
        n = t.shape[0]
        ref = t.double().sum(0)
        bound = n * 2.0 ** -24 * t.double().abs().sum(0)
        err = (sums[i].double() - ref).abs()
        assert bool((err <= bound).all()), (what, i, float((err / bound.clamp_min(1e-300)).max()))


# ------------------------------------------------------------------------------ (a) --
@pytest.mark.parametrize("name", mb.BUILDERS)
@pytest.mark.parametrize("shape", sorted(mb.SHAPES))
def test_per_point_accuracy(shape, name):
    P, ns, nb, comb = mb.SHAPES[shape]
    c = small_case(P, ns, nb, comb)
    d_o = mb.build(name, P, 5)
    got, _ = chain(c, d_o)
    g32, r32, g64, r64 = references(c, d_o)
    what = "%s %s" % (shape, name)
    worst, worst32, n_zero = check_points(what, c, got, r32, r64)
    print("MEASURED %s: kernel %.3g, fp32 torch backward %.3g, %d exactly-zero points" % (what, worst, worst32, n_zero))
    if name in ("surface", "zero_tile", "sigma_only", "rgb_only"):
        assert n_zero * 4 >= P
    check_params(what, c, d_o, g32, g64)


# ------------------------------------------------------------------------------ (b) --
@pytest.mark.parametrize("name", ["surface", "wide"])
@pytest.mark.parametrize("shape", sorted(mb.SHAPES))
def test_position_invariance_under_a_permutation(shape, name):
    P, ns, nb, comb = mb.SHAPES[shape]
    c = small_case(P, ns, nb, comb)
    d_o = mb.build(name, P, 5)
    perm = mb.hashed_perm(P, 41)
    d_o2 = torch.empty_like(d_o)
    d_o2[perm] = d_o
    a, _ = chain(c, d_o)
    b, _ = chain(c, d_o2, save=mb.permute_points(c.save, perm.to(DEV), P, nb, ns))
    assert_same_points("permuted", a, P, torch.arange(P, device=DEV), b, P, perm.to(DEV))
    assert not mb.same_bits(a["dy"][nb], b["dy"][nb])


def test_position_invariance_in_a_larger_launch():
    """The 200 points at hashed positions of a launch with CU + 1 tiles (two tiles on workgroup 0),
    ``wide`` points elsewhere, the save tiled from the small one's rows."""
    P, ns, nb, comb = mb.SHAPES["p200"]
    c = small_case(P, ns, nb, comb)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    PB = mb.TILE * (cu + 1)
    d_o = mb.build("surface", P, 5)
    pos = mb.hashed_perm(PB, 43)[:P]
    src = torch.arange(PB) % P
    src[pos] = torch.arange(P)
    d_big = mb.wide(PB, 6)
    d_big[pos] = d_o
    a, _ = chain(c, d_o)
    b, _ = chain(c, d_big, save=mb.gather_points(c.save, src.to(DEV), P, nb, ns), P=PB)
    assert_same_points("embedded", a, P, torch.arange(P, device=DEV), b, PB, pos.to(DEV))


# ------------------------------------------------------------------------------ (c) --
def edge_run(c, what):
    d_o = mb.wide(c.P, 5)
    got, sums = chain(c, d_o)
    _, r32, _, r64 = references(c, d_o)
    check_points(what, c, got, r32, r64)
    check_bias(what, c, got, sums)
    again, sums2 = chain(c, d_o)
    assert_same_run(what, got, again)
    assert mb.same_bits(sums, sums2), what


@pytest.mark.parametrize("P,ns,nb,comb", mb.EDGES, ids=["%d-%d-%d-%d" % e for e in mb.EDGES])
def test_point_count_edges(P, ns, nb, comb):
    edge_run(small_case(P, ns, nb, comb), "edge %d-%d-%d-%d" % (P, ns, nb, comb))


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("which", [0, 1], ids=["cu_plus_1_tiles_ragged", "2cu_minus_1_tiles_plus_1"])
def test_uneven_tiles_per_workgroup(which, ns):
    """64 (CU + 1) - 7 and 64 (2 CU - 1) + 1 points on a 2-block model: 1 tile on some workgroups and
    2 on others, and a ragged tile as a workgroup's second."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    P = mb.uneven_counts(cu)[which]
    edge_run(make_case(P, ns, 2, 1), "uneven %d ns %d" % (P, ns))


# ------------------------------------------------------------------------------ (d) --
@pytest.mark.parametrize("P,ns,nb,comb", mb.MASK_CASES, ids=["%d-%d-%d-%d" % e for e in mb.MASK_CASES])
def test_saved_masks_equal_the_saved_relu_signs(P, ns, nb, comb):
    c = small_case(P, ns, nb, comb)
    r = mb.save_regions(c.save, P, nb, ns)
    seen = [0, 0]
    for i, (x, m) in enumerate(zip(r["relu"], r["mask"])):
        rows = mb.relu_rows(i, P, nb, c.nc, ns)      # rows past the per-point stages' P are not written
        bits = mb.decode_masks(m[:rows])
        assert torch.equal(bits, x[:rows] > 0), (i, int((bits != (x[:rows] > 0)).sum()))
        seen[0] += int(bits.sum())
        seen[1] += int((~bits).sum())
    assert seen[0] > 0 and seen[1] > 0


def test_an_activation_of_exactly_zero_passes_no_gradient():
    """lin_in rows 16 k + k % 16, k = 0 .. 31 (every position of a lane's 16 mask bits, every
    wave) zeroed, weight and bias, in the 1-block / combine-0 model: x_0 is exactly 0 in those 32
    channels, relu(x_0) is saved as 0 with mask bit 0, and fc_0's input gradient is masked there
    (torch: relu'(0) = 0).  x_0 also reaches the output through the block's residual path, so
    dL/dx_0 = dy[nb] is not 0 there: it equals the residual path's dy[nb + 1] in those channels,
    and only there."""
    k = torch.arange(32)
    ch = 16 * k + k % 16

    def edit(mlp):
        mlp.lin_in.weight[ch] = 0.0
        mlp.lin_in.bias[ch] = 0.0

    P = 65
    c = make_case(P, 1, 1, 0, edit=edit)
    r = mb.save_regions(c.save, P, 1, 1)
    assert bool((r["relu"][0][:, ch] == 0).all())
    assert not bool(mb.decode_masks(r["mask"][0])[:, ch].any())
    d_o = mb.wide(P, 5)
    got, _ = chain(c, d_o)
    _, r32, _, r64 = references(c, d_o)
    check_points("exact zero", c, got, r32, r64)
    lin_in, fc1 = got["dy"][1], got["dy"][2]
    assert bool((lin_in[:, ch] == fc1[:, ch]).all())
    assert bool((r64["dy"][1][:, ch] == r64["dy"][2][:, ch]).all())
    other = torch.ones(512, dtype=torch.bool)
    other[ch] = False
    assert not bool((lin_in[:, other] == fc1[:, other]).all())


# ------------------------------------------------------------------------------ (e) --
@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("shape", sorted(mb.SHAPES))
def test_a_non_finite_row_stays_in_its_point(shape, kind):
    P, ns, nb, comb = mb.SHAPES[shape]
    c = small_case(P, ns, nb, comb)
    d_o, p = mb.poison(kind, P, 5)
    clean = d_o.clone()
    clean[p] = 0.0
    a, _ = chain(c, clean)
    b, _ = chain(c, d_o)
    keep = torch.cat([torch.arange(p), torch.arange(p + 1, P)]).to(DEV)
    assert_same_points("poisoned", a, P, keep, b, P, keep)
    me = torch.tensor([p], device=DEV)
    for k, ts in mb.as_lists(b).items():
        for j, t in enumerate(ts):
            rows = rows_of(t, P, me)
            assert bool((~torch.isfinite(rows)).any(1).all()), (k, j)
    for k, ts in mb.as_lists(a).items():
        for t in ts:
            assert bool(torch.isfinite(t).all()) and bool((rows_of(t, P, me) == 0).all())


# ------------------------------------------------------------------------------ (f) --
def test_an_in_place_weight_update_repacks_the_transposed_weights():
    P, ns, nb, comb = mb.SHAPES["p200"]
    c = make_case(P, ns, nb, comb)
    d_o = mb.build("wide", P, 5)
    before, _ = chain(c, d_o)
    with torch.no_grad():
        c.mlp.blocks[1].fc_1.weight.mul_(1.5)
    c.mlp.packed_t(c.net.code, "f16x3")
    c.save = forward_save(c)
    after, _ = chain(c, d_o)
    _, r32, _, r64 = references(c, d_o)
    check_points("updated weights", c, after, r32, r64)
    assert not mb.same_bits(after["dy"][1], before["dy"][1])
    assert not mb.same_bits(after["d_feat"], before["d_feat"])
