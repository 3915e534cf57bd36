"""pnr.ops.mesh_sample / nearest / mesh_distance (csrc/meshdist.hip) on the device against
tests/mesh_ref.py: the fp64 brute-force nearest neighbour, the numpy restatement of the sampling rule
on oracle/philox.py, and the fp64 score formulas.  The device ops are compared with themselves only
for run-to-run and alone-versus-together bit identity.

Bounds, with u = 2^-24 (fp32 unit roundoff) and D the exact squared distance of the fp32 inputs:
  |d2 - D(idx)| <= 6 u D(idx)     three rounded differences ((1 + u)^2 on each square), three squares
                                  and two additions of non-negative terms (the device's fma form
                                  rounds less often and stays inside)
  D(idx) <= (1 + 12 u) min_j D    the winner's fp32 d2 is at most the true nearest's fp32 d2
  points within 8 u max|vertex|   two differences, two products, two sums of terms <= 2 max|vertex|
  distance means to 1e-6 relative 3 u = 1.8e-7 per distance from the first bound
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ref
from pnr import _lib, evaluate, ops

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = mesh_ref.U
Q, B, S = ops.NEAREST_QUERIES, ops.NEAREST_TILE, ops.NEAREST_SLICE
C = ops.MESH_SCAN_CHUNK
NS = [1, Q - 1, Q + 1, 3 * Q + 5]
MS = [1, B - 1, B + 1, S + 1, 2 * S + B + 3]


def dev():
    return torch.device("cuda", 0)


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


_CLOUDS = {}


def clouds():
    """(a, b) uniform in [-1, 1]^3 at the largest sizes; the cases are prefixes."""
    if not _CLOUDS:
        rng = np.random.default_rng(20)
        _CLOUDS["a"] = rng.uniform(-1, 1, (max(NS), 3)).astype(np.float32)
        _CLOUDS["b"] = rng.uniform(-1, 1, (max(MS), 3)).astype(np.float32)
    return _CLOUDS["a"], _CLOUDS["b"]


_REF = {}


def ref_nearest(m):
    """fp64 brute force of all of a against b[:m], once per m."""
    if m not in _REF:
        a, b = clouds()
        _REF[m] = mesh_ref.nearest(a, b[:m])
    return _REF[m]


def check_nearest(a, b, dmin=None):
    d2, idx = ops.nearest(to_dev(a), to_dev(b))
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (len(a),)
    d2, idx = d2.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
    assert idx.min() >= 0 and idx.max() < len(b)
    if dmin is None:
        dmin = mesh_ref.nearest(a, b)[0]
    d_idx = mesh_ref.sqdist(a, b[idx])
    with np.errstate(invalid="ignore", divide="ignore"):
        e1 = np.where(d_idx > 0, np.abs(d2 - d_idx) / d_idx, np.abs(d2))
        e2 = np.where(dmin > 0, d_idx / dmin - 1.0, d_idx)
    print("n %d m %d: max |d2 - D|/D = %.2f u, max D(idx)/Dmin - 1 = %.2f u" % (len(a), len(b), e1.max() / U,
                                                                                e2.max() / U))
    assert (np.abs(d2 - d_idx) <= 6 * U * d_idx).all()
    assert (d_idx <= (1 + 12 * U) * dmin).all()
    return d2, idx


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_nearest_matches_the_fp64_brute_force(n, m):
    a, b = clouds()
    check_nearest(a[:n], b[:m], ref_nearest(m)[0][:n])


def test_nearest_of_near_pairs():
    """a = b + 1e-3: distances of 1e-6 at coordinates near 1, where |a|^2 + |b|^2 - 2 a.b keeps no
    digit."""
    _, b = clouds()
    b = b[:S + 1]
    rng = np.random.default_rng(21)
    a = (b[:Q + 1] + 1e-3 * rng.uniform(-1, 1, (Q + 1, 3))).astype(np.float32)
    check_nearest(a, b)


@pytest.mark.parametrize("half", [B // 2 + 1, S + 3])
def test_equal_distances_resolve_to_the_lower_index(half):
    """Every point of b twice, at j and j + m / 2; with half = S + 3 the two copies lie in different
    slices, with B / 2 + 1 in one slice and different tiles or the same."""
    rng = np.random.default_rng(22)
    pts = rng.uniform(-1, 1, (half, 3)).astype(np.float32)
    b = np.concatenate([pts, pts])
    a = np.concatenate([rng.uniform(-1, 1, (Q + 7, 3)).astype(np.float32), pts[::3]])
    d2, idx = check_nearest(a, b)
    assert idx.max() < half
    assert np.array_equal(idx[Q + 7:], np.arange(half)[::3]) and (d2[Q + 7:] == 0).all()


def test_a_cloud_against_itself():
    _, b = clouds()
    b = b[:S + 1]
    assert len(np.unique(b, axis=0)) == len(b)
    t = to_dev(b)
    d2, idx = ops.nearest(t, t)
    assert bool((d2 == 0).all()) and np.array_equal(idx.cpu().numpy(), np.arange(len(b)))


def test_nearest_is_bit_identical_from_run_to_run():
    a, b = clouds()
    ta, tb = to_dev(a), to_dev(b)
    d0, i0 = ops.nearest(ta, tb)
    d1, i1 = ops.nearest(ta, tb)
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(i0, i1)


def test_nearest_validates_its_arguments():
    t = torch.zeros(4, 3, device=dev())
    with pytest.raises(ValueError):
        ops.nearest(t.cpu(), t)
    with pytest.raises(ValueError):
        ops.nearest(t.double(), t)
    with pytest.raises(ValueError):
        ops.nearest(t[:, :2], t)
    with pytest.raises(ValueError):
        ops.nearest(t[:0], t)


# ---- sampling --------------------------------------------------------------------------------------
def one_triangle():
    return np.array([[0.1, 0.2, 0.3], [1.5, -0.2, 0.4], [0.3, 1.1, -0.9]], np.float32), np.array([[0, 1, 2]], np.int32)


def collapsed_sphere():
    v, f = mesh_ref.icosphere(2, 1.3)
    f = f.copy()
    f[::5] = f[::5, :1]            # 20 % of the faces collapsed to a point: area exactly 0
    return v, f


def wide_areas():
    """64 separate right triangles whose areas run from 1 down to 1e-6."""
    k = np.arange(64)
    side = np.sqrt(2.0 * 10.0 ** (-6.0 * k / 63.0))
    o = np.stack([3.0 * k, np.zeros(64), np.zeros(64)], -1)
    v = np.stack([o, o + np.stack([side, 0 * side, 0 * side], -1), o + np.stack([0 * side, side, 0 * side], -1)], 1)
    return v.reshape(-1, 3).astype(np.float32), np.arange(192, dtype=np.int32).reshape(-1, 3)


def grid_mesh(n_faces):
    """The first n_faces triangles of a bumpy 192 x 192 height field."""
    k = 192
    rng = np.random.default_rng(5)
    x, y = np.meshgrid(np.linspace(-1, 1, k + 1), np.linspace(-1, 1, k + 1), indexing="ij")
    v = np.stack([x, y, 0.02 * rng.standard_normal(x.shape)], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(k)[:, None] * (k + 1) + np.arange(k)[None, :]).reshape(-1)
    f = np.stack([np.stack([i, i + k + 1, i + 1], -1), np.stack([i + 1, i + k + 1, i + k + 2], -1)], 1).reshape(-1, 3)
    assert len(f) >= n_faces
    return v, f[:n_faces].astype(np.int32)


# seeds at which the restatement has no sample within T * 2^-52 * total of a CDF boundary (asserted)
MESHES = {
    "one_triangle": (one_triangle, 1),
    "collapsed_sphere": (collapsed_sphere, 2),
    "wide_areas": (wide_areas, 3),
    "chunk_plus_1": (lambda: grid_mesh(C + 1), 4),
    "chunk2_plus_1": (lambda: grid_mesh(C * C + 1), 5),
}


@pytest.mark.parametrize("n", [1, 4097])
@pytest.mark.parametrize("name", list(MESHES))
def test_sampling_matches_the_restatement(name, n):
    make, seed = MESHES[name]
    v, f = make()
    ref = mesh_ref.sample(v, f, n, seed)
    assert ref["near_boundary"] == 0, "pick another seed: the restatement has a draw on a CDF boundary"
    p, nrm, tri, area = ops.mesh_sample(to_dev(v), to_dev(f), n, seed=seed)
    assert p.shape == nrm.shape == (n, 3) and tri.shape == (n,) and tri.dtype == torch.int32
    assert area.dtype == torch.float64 and area.dim() == 0
    p, nrm, tri, area = p.cpu().numpy(), nrm.cpu().numpy(), tri.cpu().numpy().astype(np.int64), float(area)
    print("%s n %d: total %.17g (ref %.17g), max point error %.2f u max|v|, max normal error %.2e" % (
        name, n, area, ref["total"], np.abs(p - ref["points"]).max() / (U * np.abs(v).max()),
        np.abs(nrm - ref["normals"]).max()))
    assert abs(area - ref["total"]) <= 1e-12 * ref["total"]
    assert (ref["area"][tri] > 0).all()
    assert np.array_equal(tri, ref["tri"])
    assert np.abs(p - ref["points"]).max() <= 8 * U * np.abs(v).max()
    assert np.abs(nrm - ref["normals"]).max() < 1e-6
    _, no_normals, tri2, _ = ops.mesh_sample(to_dev(v), to_dev(f), n, seed=seed, want_normals=False)
    assert no_normals is None and np.array_equal(tri2.cpu().numpy(), tri)


def test_a_sample_depends_on_seed_and_index_only():
    v, f = collapsed_sphere()
    tv, tf = to_dev(v), to_dev(f)
    long = ops.mesh_sample(tv, tf, 4097, seed=9)
    short = ops.mesh_sample(tv, tf, 100, seed=9)
    again = ops.mesh_sample(tv, tf, 4097, seed=9)
    other = ops.mesh_sample(tv, tf, 100, seed=10)
    for k in range(3):
        assert torch.equal(long[k][:100].view(torch.int32), short[k].view(torch.int32))
        assert torch.equal(long[k].view(torch.int32), again[k].view(torch.int32))
    assert torch.equal(long[3].view(torch.int64), short[3].view(torch.int64))
    assert not torch.equal(other[2], short[2])


def test_bad_meshes_are_refused_by_the_check():
    v, f = mesh_ref.icosphere(1)
    bad = f.copy()
    bad[17, 1] = len(v)                       # one past the last vertex
    with pytest.raises(_lib.PnrError, match="outside"):
        ops.mesh_sample(to_dev(v), to_dev(bad), 64)
    bad[17, 1] = -1
    with pytest.raises(_lib.PnrError, match="outside"):
        ops.mesh_sample(to_dev(v), to_dev(bad), 64)
    flat = np.zeros_like(f)                   # every face a point: total area 0
    with pytest.raises(_lib.PnrError, match="total area"):
        ops.mesh_sample(to_dev(v), to_dev(flat), 64)
    # the device is intact: the next call works
    p, _, _, _ = ops.mesh_sample(to_dev(v), to_dev(f), 64)
    assert bool(torch.isfinite(p).all())
    with pytest.raises(ValueError):
        ops.mesh_sample(to_dev(v), to_dev(f).long(), 64)
    with pytest.raises(ValueError):
        ops.mesh_sample(to_dev(v), to_dev(f), 0)


# ---- scores ----------------------------------------------------------------------------------------
_SCORE = {}


def score_inputs():
    """Device samples of two concentric spheres (more than one slice of b), and mesh_ref's fp64 scores
    of those very points, once."""
    if not _SCORE:
        vi, fi = mesh_ref.icosphere(3, 1.0)
        vo, fo = mesh_ref.icosphere(3, 1.1)
        pa, na, _, _ = ops.mesh_sample(to_dev(vi), to_dev(fi), 3001, seed=31)
        pb, nb, _, _ = ops.mesh_sample(to_dev(vo), to_dev(fo), S + 905, seed=32)
        tau = 0.104        # near the median of both distance fields
        ref, d_ab, d_ba = mesh_ref.scores(pa.cpu().numpy(), na.cpu().numpy(), pb.cpu().numpy(), nb.cpu().numpy(), tau)
        _SCORE.update(pa=pa, na=na, pb=pb, nb=nb, tau=tau, ref=ref, d_ab=d_ab, d_ba=d_ba)
    return _SCORE


def test_scores_match_the_fp64_formulas():
    s = score_inputs()
    got = ops.mesh_distance(s["pa"], s["na"], s["pb"], s["nb"], s["tau"])
    assert set(got) == set(ops.MESH_DISTANCE_KEYS) == set(evaluate.MESH_METRIC_NAMES)
    for k, t in got.items():
        assert t.dtype == torch.float64 and t.dim() == 0 and t.device.type == "cuda"
    got = {k: float(t) for k, t in got.items()}
    ref, tau = s["ref"], s["tau"]
    for k in got:
        print("%-22s %.12g ref %.12g" % (k, got[k], ref[k]))
    # the reference has no distance within 3 u tau of tau, so the counts must agree exactly
    for d in (s["d_ab"], s["d_ba"]):
        assert int((np.abs(d - tau) <= 3 * U * tau).sum()) == 0, "pick another tau"
    n, m = len(s["d_ab"]), len(s["d_ba"])
    assert 0.2 < ref["precision"] < 0.8 and 0.2 < ref["recall"] < 0.8       # tau cuts through the distances
    assert round(got["precision"] * n) == round(ref["precision"] * n)
    assert round(got["recall"] * m) == round(ref["recall"] * m)
    for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2"):
        assert abs(got[k] - ref[k]) <= 1e-6 * ref[k], k
    assert abs(got["fscore"] - ref["fscore"]) <= 1e-12
    for k in ("normals_accuracy", "normals_completeness", "normal_consistency"):
        assert abs(got[k] - ref[k]) <= 1e-6, k
    none = ops.mesh_distance(s["pa"], None, s["pb"], None, tau)
    assert float(none["normal_consistency"]) == 0.0 and float(none["accuracy"]) == got["accuracy"]


def test_score_sums_are_bit_identical_across_runs_and_calls():
    s = score_inputs()
    d2_ab, i_ab = ops.nearest(s["pa"], s["pb"])
    d2_ba, i_ba = ops.nearest(s["pb"], s["pa"])
    one = ops.mesh_distance_sums(d2_ab, i_ab, d2_ba, i_ba, s["na"], s["nb"], s["tau"])
    two = ops.mesh_distance_sums(d2_ab, i_ab, d2_ba, i_ba, s["na"], s["nb"], s["tau"])
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))
    # a direction's sums do not depend on what is scored with it: the clouds exchanged ...
    swapped = ops.mesh_distance_sums(d2_ba, i_ba, d2_ab, i_ab, s["nb"], s["na"], s["tau"])
    assert torch.equal(swapped[4:].view(torch.int64), one[:4].view(torch.int64))
    assert torch.equal(swapped[:4].view(torch.int64), one[4:].view(torch.int64))
    # ... and beside a seven-point stub (no normals: the stub's indices would not match)
    alone = ops.mesh_distance_sums(d2_ab, i_ab, d2_ba, i_ba, None, None, s["tau"])
    stub = ops.mesh_distance_sums(d2_ab, i_ab, d2_ba[:7].contiguous(), i_ba[:7].contiguous(), None, None, s["tau"])
    assert torch.equal(stub[:3].view(torch.int64), alone[:3].view(torch.int64))
    assert torch.equal(alone[:3].view(torch.int64), one[:3].view(torch.int64))
    assert float(alone[3]) == 0.0 and float(alone[7]) == 0.0


# ---- callers ---------------------------------------------------------------------------------------
def test_mesh_metrics_backends_agree():
    """The same Philox rule and the same seed on both backends: the same samples, so the scores differ
    by the fp32 distances only (1e-6 relative); a precision / recall count may move by the points
    within 3 u tau of tau, at most 2 per 10,000."""
    n = 20000
    inner, outer = mesh_ref.icosphere(3, 1.0), mesh_ref.icosphere(3, 1.1)
    host = evaluate.mesh_metrics(inner, outer, n_samples=n, tau=0.104, seed=3, backend="numpy")
    hip = evaluate.mesh_metrics(inner, outer, n_samples=n, tau=0.104, seed=3, backend="hip")
    on_dev = evaluate.mesh_metrics(tuple(to_dev(x) for x in inner), tuple(to_dev(x) for x in outer), n_samples=n,
                                   tau=0.104, seed=3, backend="auto")
    assert on_dev == hip
    for k in evaluate.MESH_METRIC_NAMES:
        print("%-22s hip %.12g numpy %.12g" % (k, hip[k], host[k]))
    for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2"):
        assert abs(hip[k] - host[k]) <= 1e-6 * host[k], k
    for k in ("precision", "recall"):
        assert abs(hip[k] - host[k]) * n <= 2 * n / 10000, k
    for k in ("normals_accuracy", "normals_completeness", "normal_consistency"):
        assert abs(hip[k] - host[k]) <= 1e-6, k
    sag, spacing = mesh_ref.sphere_slack(3, 1.1, n)
    assert 0.1 - sag - spacing <= hip["accuracy"] <= 0.1 + sag + spacing


def test_eval_mesh_script_hip_backend(tmp_path):
    n, res = 4000, 33
    out, gt = mesh_ref.write_eval_tree(str(tmp_path), res, {"a": (0.5, 3.0), "b": (0.4, 1.0), "c": (0.5, None)})
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "scripts", "eval_mesh.py"), "-O", out,
           "-G", gt, "--mesh_res", str(res), "--normalize", "gt", "--gt_radius", "0.55", "--n_samples", str(n),
           "--tau", "0.1", "--seed", "5", "--metrics_backend", "hip"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Scoring with the hip backend" in r.stdout and r.stderr.count("skipped") == 1
    sag, spacing = mesh_ref.sphere_slack(3, 0.55, n)
    s = sag + spacing + 2.0 / (res - 1) * 2.0 ** -20
    for k, gap in (("a", 0.05), ("b", 0.15)):
        with open(os.path.join(out, k, "mesh_metrics.txt")) as fh:
            row = {name: float(x) for name, x in (ln.split() for ln in fh)}
        assert list(row) == list(evaluate.MESH_METRIC_NAMES)
        assert gap - s <= row["accuracy"] <= gap + s and gap - s <= row["completeness"] <= gap + s
    assert open(os.path.join(out, "all_mesh_metrics.txt")).read().endswith("objects 2\n")


def test_eval_script_scores_the_device_mesh(tmp_path):
    """scripts/eval.py --mesh_backend hip --gt_mesh_dir on the synthetic SRN set: mesh_metrics.txt
    beside every STL whose object has a ground truth, one stderr line for the one that has none."""
    from pnr import mesh
    from pnr.data import get_split_dataset
    from test_gpu_mcubes import DEV, _eval_module, _synth_setup

    root, net = _synth_setup(tmp_path)
    dset = get_split_dataset("srn", root, want_split="test", training=False)
    names = [os.path.basename(dset[i]["path"]) for i in range(len(dset))]
    assert len(names) >= 2
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
    for name in names[:-1]:                   # the last object has no ground truth
        mesh.write_stl(str(gt / (name + ".stl")), v, f)
    out = tmp_path / "out"
    r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, os.path.join(REPO, "scripts", "eval.py"), "-c",
                        str(tmp_path / "exp.conf"), "-D", root, "-n", "synthnet", "--checkpoints_path",
                        str(tmp_path / "ck"), "--split", "test", "-P", "0 1", "--mesh_res", "20", "--mesh_thresh",
                        repr(thresh), "--mesh_backend", "hip", "--gt_mesh_dir", str(gt), "--n_samples", "5000",
                        "-O", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ERROR" not in r.stdout, r.stdout[-3000:]
    assert r.stderr.count("no ground truth") == 1 and names[-1] in r.stderr
    assert not (out / names[-1] / "mesh_metrics.txt").exists()
    for i, name in enumerate(names[:-1]):
        assert (out / name / (name + "_mesh.stl")).exists()
        with open(str(out / name / "mesh_metrics.txt")) as fh:
            row = {k: float(x) for k, x in (ln.split() for ln in fh)}
        assert list(row) == list(evaluate.MESH_METRIC_NAMES)
        if i == 0:   # the threshold is the median of this object's densities: it has a surface
            assert all(np.isfinite(x) for x in row.values()) and row["chamfer_l1"] > 0
            # The STL holds the same faces in the same order, so the host route draws the same
            # samples from it; the two differ by the fp32 rounding of the transforms (1e-7
            # relative), which moves a distance by as much and, rarely, one sample in 5,000 to a
            # neighbouring face (2e-4 of the mean at most): 1e-3 relative.
            pv, pf = mesh.read_stl_indexed(str(out / name / (name + "_mesh.stl")))
            again = evaluate.mesh_metrics((mesh.normalize_bounds(pv * (2.0 / 19) - 1.0), pf),
                                          (mesh.normalize_bounds(v), f), n_samples=5000, backend="numpy")
            print(row, again)
            assert abs(again["chamfer_l1"] - row["chamfer_l1"]) <= 1e-3 * row["chamfer_l1"]
