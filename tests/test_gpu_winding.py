"""pnr.ops.winding_number / mesh_contains / box_sample (csrc/winding.hip) and the hip backend of
pnr.evaluate.volume_iou on the device, against tests/winding_ref.py's fp64 restatement of the formula
(winding64) and oracle/philox.py.  The device ops are compared with themselves only for run-to-run,
alone-versus-together and bad-face bit identity.

The bound.  winding32, the host emulation of the device's fp32 pair arithmetic (the same roundings
and fmas, numpy's atan2f), was compared with winding64 when the bound was set: at most 2.7e-7 in w
over icospheres of 320 / 1,280 / 5,120 faces (one translated by 37, one of radius 0.3), each with
3,000 uniform queries, 150 within 1e-3 of the surface and 50 on vertices.  The device differs from
the emulation in atan2f (a few ulp), so it is held to 1e-6 against winding64, about 4 x the
emulation's own error.  Every test prints its measured maximum; on one MI355X the largest is 7.1e-7
(the closed sphere at (37, -5, 11); the emulation gives 7.1e-7 on the same queries), 6.1e-8 on the
open prefixes and 4.7e-8 at the grid points of the marching-cubes surfaces.  "Within 1e-3 of the
surface" is read as within 1e-3 of the sphere the icosphere is inscribed in; queries as near to the
faces themselves come as near to an edge, where the fp32 rule loses digits (test_queries_hugging_
the_faces_classify says how many and why), and are held to the classification.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mc_ref
import mesh_ref
import winding_ref
from oracle import philox
from pnr import _lib, evaluate, ops

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, T, S = ops.WINDING_QUERIES, ops.WINDING_TILE, ops.WINDING_SLICE
NS = [1, Q - 1, Q + 1, 2 * Q + 5]
MS = [1, T - 1, T + 1, S + 1, 2 * S + T + 3]
BOUND = 1e-6


def dev():
    return torch.device("cuda", 0)


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def winding(v, f, p):
    w = ops.winding_number(to_dev(v), to_dev(f), to_dev(p))
    assert w.dtype == torch.float64 and w.shape == (len(p),) and w.device.type == "cuda"
    return w.cpu().numpy()


def bits(w):
    return np.asarray(w, np.float64).view(np.int64)


_DATA = {}


def sphere5():
    if "mesh" not in _DATA:
        _DATA["mesh"] = mesh_ref.icosphere(5 if max(MS) <= 20480 else 6)
        _DATA["queries"] = np.random.default_rng(50).uniform(-1.25, 1.25, (max(NS), 3)).astype(np.float32)
    return _DATA["mesh"], _DATA["queries"]


def ref_open(m):
    """winding64 of all the queries against the first m faces, once per m."""
    if ("ref", m) not in _DATA:
        (v, f), q = sphere5()
        _DATA["ref", m] = winding_ref.winding64(v, f[:m], q)
    return _DATA["ref", m]


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_open_meshes_match_the_fp64_formula(n, m):
    """The first m faces of an icosphere (an open mesh: fractional w) at the tile, slice and
    workgroup edges."""
    (v, f), q = sphere5()
    assert len(f) >= m
    w = winding(v, f[:m], q[:n])
    e = np.abs(w - ref_open(m)[:n]).max()
    print("n %d m %d: max |w - w64| = %.3g" % (n, m, e))
    assert e <= BOUND


def closed_case():
    """icosphere(3) at (37, -5, 11); 3,000 uniform queries, 150 within 1e-3 of the sphere it is
    inscribed in, and (kept apart) 150 within 1e-3 of the faces themselves."""
    if "closed" not in _DATA:
        off = np.array([37, -5, 11], np.float32)
        v, f = mesh_ref.icosphere(3)
        v = v + off
        rng = np.random.default_rng(51)
        p = np.concatenate([rng.uniform(-1.25, 1.25, (3000, 3)).astype(np.float32) + off,
                            winding_ref.near_sphere(off, 1.0, 150, 1e-3, rng)])
        hug = winding_ref.near_faces(v, f, 150, 1e-3, rng)
        _DATA["closed"] = (v, f, p, winding_ref.winding64(v, f, p), hug, winding_ref.winding64(v, f, hug))
    return _DATA["closed"]


def test_closed_mesh_classification():
    v, f, p, w64, _, _ = closed_case()
    w = winding(v, f, p)
    e = np.abs(w - w64).max()
    sure = np.abs(w64 - 0.5) >= 1e-3
    print("closed sphere at (37, -5, 11): max |w - w64| = %.3g, %d of %d queries within 1e-3 of 0.5" % (
        e, int((~sure).sum()), len(p)))
    assert e <= BOUND
    assert (~sure).sum() <= 0.01 * len(p)
    inside = ops.mesh_contains(to_dev(v), to_dev(f), to_dev(p))
    assert inside.dtype == torch.bool and inside.shape == (len(p),)
    assert np.array_equal(inside.cpu().numpy()[sure], (w64 > 0.5)[sure])
    assert 0.2 < (w64 > 0.5).mean() < 0.8
    # another threshold is the same comparison
    assert np.array_equal(ops.mesh_contains(to_dev(v), to_dev(f), to_dev(p), 0.25).cpu().numpy(), w > 0.25)


def test_queries_hugging_the_faces_classify():
    """Queries within 1e-3 of the faces themselves, some as near to an edge.  There the fp32 pair rule
    is ill-conditioned: num and den are both about (distance to the edge / edge length) |a||b||c|,
    their rounding errors about 2^-24 |a||b||c|, so a face's angle is off by about 2^-24 x edge
    length / distance, 1e-5 rad at 1e-3 of an edge of 0.15, which the emulation (winding32) shows as
    well.  That is far from moving w across 0.5: the classification is asserted, and w to 1e-4."""
    v, f, _, _, hug, w64 = closed_case()
    w = winding(v, f, hug)
    sure = np.abs(w64 - 0.5) >= 1e-3
    print("150 queries within 1e-3 of the faces: max |w - w64| = %.3g, %d within 1e-3 of 0.5" % (
        np.abs(w - w64).max(), int((~sure).sum())))
    assert (~sure).sum() <= 0.01 * len(hug)
    assert np.array_equal((w > 0.5)[sure], (w64 > 0.5)[sure])
    assert np.abs(w - w64).max() <= 1e-4


def test_queries_on_vertices_are_finite():
    v, f = closed_case()[:2]
    w = winding(v, f, v[:50])
    print("on 50 vertices: w in [%.9g, %.9g]" % (w.min(), w.max()))
    assert np.isfinite(w).all() and w.min() >= -1e-6 and w.max() <= 1 + 1e-6


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_grid_points_against_the_marching_cubes_surface(name):
    """Every grid point is collinear with mesh vertices (they lie on the grid lines): the case that
    breaks ray parity.  The surface is closed (the border is below the level), and no grid value is
    within 5e-4 of the level, so w is the indicator of grid > 0 at every grid point."""
    if name == "sphere":
        shape, inside_count = (20, 18, 16), 600
        grid = mc_ref.sphere_grid(shape, (9.3, 8.6, 7.4), 5.2)
    else:
        shape, inside_count = (24, 24, 12), 802
        grid = mc_ref.torus_grid(shape, (11.4, 11.7, 5.3), 6.1, 2.6)
    assert np.abs(grid).min() >= 5e-4
    border = np.ones(shape, bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert grid[border].max() < -2.2
    assert int((grid > 0).sum()) == inside_count
    verts, faces = ops.marching_cubes(to_dev(grid), 0.0)
    assert mc_ref.is_closed_oriented(faces.cpu().numpy())
    pts = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    w = ops.winding_number(verts, faces, to_dev(pts)).cpu().numpy()
    e = np.abs(w - (grid.reshape(-1) > 0)).max()
    print("%s: %d faces, %d grid points, max |w - (grid > 0)| = %.3g" % (name, faces.shape[0], len(pts), e))
    assert e <= BOUND
    assert np.array_equal(ops.mesh_contains(verts, faces, to_dev(pts)).cpu().numpy(), grid.reshape(-1) > 0)


def test_faces_with_bad_indices_contribute_nothing():
    (v, f), q = sphere5()
    q = q[:Q + 1]
    # one slice: the bad faces anywhere
    good = f[:S - 40]
    bad = good.copy()
    rows = np.arange(3, len(bad), 97)
    bad[rows[0::2], 1] = -1
    bad[rows[1::2], 2] = len(v)
    keep = np.ones(len(bad), bool)
    keep[rows] = False
    assert np.array_equal(bits(winding(v, bad, q)), bits(winding(v, good[keep], q)))
    # several slices: a bad face keeps its place, like a face that is a point; trailing ones vanish
    many = f[:2 * S + T + 3].copy()
    rows = np.arange(5, len(many), 211)
    point = many.copy()
    point[rows] = 0
    many[rows, 0] = np.where(np.arange(len(rows)) % 2 == 0, -1, len(v))
    w_bad = winding(v, many, q)
    assert np.array_equal(bits(w_bad), bits(winding(v, point, q)))
    tail = np.concatenate([many, np.full((T + 9, 3), len(v), np.int32), np.full((3, 3), -7, np.int32)])
    assert np.array_equal(bits(winding(v, tail, q)), bits(w_bad))
    keep = np.ones(len(many), bool)
    keep[rows] = False
    assert np.abs(w_bad - winding_ref.winding64(v, many[keep], q)).max() <= BOUND
    # the vertices of a bad face are never read: a mesh of bad faces only, with a one-vertex buffer
    w0 = ops.winding_number(torch.zeros(1, 3, device=dev()), to_dev(np.full((5, 3), 1, np.int32)), to_dev(q))
    assert bool((w0 == 0).all())


def test_non_finite_inputs_give_nan():
    v, f, p = closed_case()[:3]
    p = p[:2 * Q + 5].copy()
    clean = winding(v, f, p)
    dirty = p.copy()
    dirty[[0, Q - 1, Q + 3], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    w = winding(v, f, dirty)
    hit = np.zeros(len(p), bool)
    hit[[0, Q - 1, Q + 3]] = True
    assert np.isnan(w[hit]).all()
    assert np.array_equal(bits(w[~hit]), bits(clean[~hit]))
    inside = ops.mesh_contains(to_dev(v), to_dev(f), to_dev(dirty)).cpu().numpy()
    assert not inside[hit].any() and np.array_equal(inside[~hit], clean[~hit] > 0.5)
    # a used vertex that is not finite: every w is NaN
    for val in (np.nan, np.inf):
        vb = v.copy()
        vb[f[7, 1], 2] = val
        assert np.isnan(winding(vb, f, p[:Q + 1])).all()
    # an unused one changes nothing
    vb = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)
    assert np.array_equal(bits(winding(vb, f, p)), bits(clean))


def test_winding_is_bit_identical_across_runs_and_batches():
    (v, f), q = sphere5()
    m = 2 * S + T + 3
    tv, tf, tq = to_dev(v), to_dev(f[:m]), to_dev(q)
    one, two = ops.winding_number(tv, tf, tq), ops.winding_number(tv, tf, tq)
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))
    alone = ops.winding_number(tv, tf, tq[:Q - 1].contiguous())
    assert torch.equal(alone.view(torch.int64), one[:Q - 1].view(torch.int64))
    # a row's position does not matter either
    moved = ops.winding_number(tv, tf, torch.flip(tq, [0]).contiguous())
    assert torch.equal(torch.flip(moved, [0]).view(torch.int64), one.view(torch.int64))


def test_winding_validates_its_arguments():
    v, f = mesh_ref.icosphere(0)
    tv, tf, tp = to_dev(v), to_dev(f), torch.zeros(4, 3, device=dev())
    with pytest.raises(ValueError):
        ops.winding_number(tv.cpu(), tf, tp)
    with pytest.raises(ValueError):
        ops.winding_number(tv, tf.long(), tp)
    with pytest.raises(ValueError):
        ops.winding_number(tv, tf, tp.double())
    with pytest.raises(ValueError):
        ops.winding_number(tv, tf, tp[:, :2])
    with pytest.raises(ValueError):
        ops.winding_number(tv, tf, tp[:0])
    with pytest.raises(ValueError):
        ops.winding_number(tv, tf[:0], tp)
    with pytest.raises(TypeError):
        ops.winding_number(v, tf, tp)


# ---- box samples -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 2 ** 40 + 3])
def test_box_sample_around_the_origin_is_the_philox_stream(seed):
    """A box that holds the origin: no coordinate is larger than its axis' extent, so the one rounding
    of fma(u, extent, lo) (and that of the extent) stays within one fp32 ulp of the extent."""
    lo, hi = np.array([-1.5, -0.3, -2.0], np.float32), np.array([0.25, 0.9, 2.5], np.float32)
    n = 4097
    p = ops.box_sample(lo.tolist(), hi.tolist(), n, seed=seed, device=dev()).cpu().numpy()
    assert (p >= lo).all() and (p <= hi).all()
    ext = (hi - lo).astype(np.float64)
    want = lo.astype(np.float64) + philox.stream(seed, 0, 5, n, 3).astype(np.float64) * ext
    ulp = 2.0 ** (np.floor(np.log2(ext)) - 23)
    err = np.abs(p - want)
    print("seed %d: max error %s of an ulp of the extent" % (seed, (err / ulp).max(0)))
    assert (err <= ulp).all()
    assert np.array_equal(p, evaluate.box_sample_np(lo, hi, n, seed))


@pytest.mark.parametrize("seed", [0, 2 ** 40 + 3])
def test_box_sample_far_from_the_origin(seed):
    """A translated box with one flat axis: here the rounding of the result, half an ulp of a value as
    large as the bounds, is what remains."""
    lo, hi = np.array([-1.5, 2.0, 36.0], np.float32), np.array([0.25, 2.0, 38.5], np.float32)
    n = 4097
    p = ops.box_sample(lo.tolist(), hi.tolist(), n, seed=seed, device=dev())
    assert p.dtype == torch.float32 and p.shape == (n, 3) and p.device.type == "cuda"
    short = ops.box_sample(lo.tolist(), hi.tolist(), 100, seed=seed, device=dev())
    assert torch.equal(short.view(torch.int32), p[:100].view(torch.int32))
    p = p.cpu().numpy()
    assert (p >= lo).all() and (p <= hi).all() and (p[:, 1] == 2.0).all()
    u = philox.stream(seed, 0, 5, n, 3).astype(np.float64)
    ext = (hi - lo).astype(np.float64)
    want = lo.astype(np.float64) + u * ext
    err = np.abs(p - want)
    # one rounding of the result: half an ulp of a value no larger than max(|lo|, |hi|)
    ulp = 2.0 ** -23 * np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
    print("seed %d: max error %s of an ulp of the bounds" % (seed, (err / ulp).max(0)))
    assert (err <= ulp).all()
    # the host route draws the same points (up to fp32 ties of its fp64 sum: none here)
    assert np.array_equal(p, evaluate.box_sample_np(lo, hi, n, seed))


def test_box_sample_validates_its_arguments():
    with pytest.raises(_lib.PnrError, match="bounds"):
        ops.box_sample([0, 0, 0], [1, -1, 1], 8, device=dev())
    with pytest.raises(_lib.PnrError, match="bounds"):
        ops.box_sample([0, 0, 0], [1, float("inf"), 1], 8, device=dev())
    with pytest.raises(ValueError):
        ops.box_sample([0, 0, 0], [1, 1, 1], 0, device=dev())
    with pytest.raises(ValueError):
        ops.box_sample([0, 0], [1, 1, 1], 8, device=dev())
    with pytest.raises(ValueError):
        ops.box_sample([0, 0, 0], [1, 1, 1], 8, device="cpu")


# ---- callers ---------------------------------------------------------------------------------------
def test_volume_iou_backends_agree():
    """Concentric spheres: no drawn point has a w within 1e-3 of 0.5 for either mesh (asserted on the
    host from winding64), so the device's occupancies, hence its integer counts, are the host's."""
    pred, gt = mesh_ref.icosphere(3, 0.8), mesh_ref.icosphere(3, 1.0)
    n, seed = 20000, 0
    both = np.concatenate([pred[0], gt[0]])
    lo, hi = evaluate._grown_box(both.min(0), both.max(0), 0.05)
    pts = evaluate.box_sample_np(lo, hi, n, seed)
    occ = []
    for v, f in (pred, gt):
        w64 = winding_ref.winding64(v, f, pts)
        assert int((np.abs(w64 - 0.5) < 1e-3).sum()) == 0
        occ.append(w64 > 0.5)
    inter, union = int((occ[0] & occ[1]).sum()), int((occ[0] | occ[1]).sum())
    host = evaluate.volume_iou(pred, gt, n_points=n, seed=seed, backend="numpy")
    hip = evaluate.volume_iou(pred, gt, n_points=n, seed=seed, backend="hip")
    on_dev = evaluate.volume_iou(tuple(to_dev(t) for t in pred), tuple(to_dev(t) for t in gt), n_points=n, seed=seed)
    print("hip", hip, "numpy", host, "counts", inter, union)
    box = float(np.prod(hi.astype(np.float64) - lo))
    assert list(hip) == list(evaluate.VOLUME_METRIC_NAMES) and all(type(x) is float for x in hip.values())
    assert hip == on_dev
    assert abs(hip["iou"] - inter / union) <= 1e-12 and abs(host["iou"] - inter / union) <= 1e-12
    assert round(hip["volume_gt"] / box * n) == int(occ[1].sum()) == round(host["volume_gt"] / box * n)
    assert round(hip["volume_pred"] / box * n) == int(occ[0].sum()) == round(host["volume_pred"] / box * n)
    assert abs(hip["iou"] - 0.512) <= 0.027
    # inward faces score as the solid they bound; an empty prediction is a result
    flipped = (gt[0], np.ascontiguousarray(gt[1][:, ::-1]))
    assert evaluate.volume_iou(pred, flipped, n_points=n, seed=seed, backend="hip") == hip
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    r = evaluate.volume_iou(empty, gt, n_points=500, backend="hip")
    assert r["iou"] == 0.0 and r["volume_pred"] == 0.0 and r["volume_gt"] > 0
    with pytest.raises(ValueError):
        evaluate.volume_iou(gt, empty, n_points=500, backend="hip")


def _read(path):
    with open(path) as fh:
        return {k: float(x) for k, x in (ln.split() for ln in fh)}


def test_eval_mesh_script_iou_backends_agree(tmp_path):
    n, res = 1500, 33
    rows = {}
    for backend in ("numpy", "hip"):
        out, gt = mesh_ref.write_eval_tree(str(tmp_path / backend), res, {"a": (0.5, 3.0), "b": (0.4, 1.0)})
        cmd = [sys.executable, os.path.join(REPO, "scripts", "eval_mesh.py"), "-O", out, "-G", gt, "--mesh_res",
               str(res), "--normalize", "gt", "--gt_radius", "0.55", "--n_samples", str(n), "--tau", "0.1", "--seed", "5",
               "--iou", "--n_iou_points", "3000", "--metrics_backend", backend]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        rows[backend] = {k: _read(os.path.join(out, k, "mesh_metrics.txt")) for k in ("a", "b")}
        allm = _read(os.path.join(out, "all_mesh_metrics.txt"))
        assert list(allm) == list(evaluate.MESH_METRIC_NAMES) + list(evaluate.VOLUME_METRIC_NAMES) + ["objects"]
        assert allm["iou"] == (0.0 + rows[backend]["a"]["iou"] + rows[backend]["b"]["iou"]) / 2
    for k, radius in (("a", 0.5), ("b", 0.4)):
        print(k, rows["hip"][k]["iou"], rows["numpy"][k]["iou"])
        assert abs(rows["hip"][k]["iou"] - rows["numpy"][k]["iou"]) <= 1e-9
        assert abs(rows["hip"][k]["iou"] - (radius / 0.55) ** 3) <= 0.1


def test_eval_script_iou_from_the_device_mesh(tmp_path):
    """scripts/eval.py --mesh_backend hip --gt_mesh_dir --iou on the synthetic SRN set: the volume lines
    follow the surface scores in mesh_metrics.txt, scored from the device tensors.  The ground truth
    is a sphere brought to radius 1 (--normalize both), so volume_gt is that polyhedron's volume up to
    the sampling error: about 0.38 of 3,000 points inside, sigma 2.3 % of the volume, the bound 15 %."""
    from pnr import mesh
    from pnr.data import get_split_dataset
    from test_gpu_mcubes import DEV, _eval_module, _synth_setup

    root, net = _synth_setup(tmp_path)
    dset = get_split_dataset("srn", root, want_split="test", training=False)
    names = [os.path.basename(dset[i]["path"]) for i in range(len(dset))]
    ev = _eval_module()
    net = net.to(DEV).eval()
    data = dset[0]
    with torch.no_grad():
        net.encode(data["images"][:2].to(DEV)[None], data["poses"][:2].to(DEV)[None],
                   torch.as_tensor(data["focal"], dtype=torch.float32)[None].to(DEV), c=data["c"].to(DEV)[None])
    sig0 = ev.density_grid(net, 20, DEV).cpu().numpy()
    thresh = float(np.median(sig0[sig0 > 0]))
    gt = tmp_path / "gt"
    gt.mkdir()
    v, f = mesh_ref.icosphere(2, 0.8)
    mesh.write_stl(str(gt / (names[0] + ".stl")), v, f)
    out = tmp_path / "out"
    r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, os.path.join(REPO, "scripts", "eval.py"), "-c",
                        str(tmp_path / "exp.conf"), "-D", root, "-n", "synthnet", "--checkpoints_path",
                        str(tmp_path / "ck"), "--split", "test", "-P", "0 1", "--mesh_res", "20", "--mesh_thresh",
                        repr(thresh), "--mesh_backend", "hip", "--gt_mesh_dir", str(gt), "--n_samples", "2000",
                        "--iou", "--n_iou_points", "3000", "-O", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ERROR" not in r.stdout, r.stdout[-3000:]
    assert " iou " in r.stdout
    row = _read(str(out / names[0] / "mesh_metrics.txt"))
    assert list(row) == list(evaluate.MESH_METRIC_NAMES) + list(evaluate.VOLUME_METRIC_NAMES)
    vol = mc_ref.signed_volume(*mesh_ref.icosphere(2, 1.0))
    print(row)
    assert 0.0 <= row["iou"] <= 1.0 and row["n_points"] == 3000.0 and row["volume_pred"] >= 0.0
    assert abs(row["volume_gt"] - vol) <= 0.15 * vol
