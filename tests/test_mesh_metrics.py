"""Host side of the mesh metrics (no GPU): the refusals of the five ABI entries through the ctypes
binding, pnr.evaluate.mesh_metrics on its numpy backend, the STL / bounds helpers of pnr.mesh and
scripts/eval_mesh.py end to end.  The device kernels are tests/test_gpu_meshdist.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref
from mesh_ref import _read
from oracle import philox
from pnr import _lib, evaluate, mesh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


def test_abi_entries_refuse_empty_and_null_arguments():
    lib = _lib.load()
    err = lib.pnr_last_error
    # sizes of 0
    assert lib.pnr_nearest(None, 0, None, 0, None, 0, None, None, None) == INVALID and b"pnr_nearest" in err()
    assert lib.pnr_mesh_sample(None, 0, None, 0, 0, 0, None, 0, None, None, None, None, None) == INVALID
    assert b"pnr_mesh_sample" in err()
    assert lib.pnr_mesh_distance_reduce(None, None, 0, None, None, 0, None, None, 0.01, None, None) == INVALID
    assert b"pnr_mesh_distance_reduce" in err()
    # NULL required pointers at valid sizes
    assert lib.pnr_nearest(None, 4, None, 4, None, 0, None, None, None) == INVALID and b"NULL" in err()
    assert lib.pnr_mesh_sample(None, 3, None, 1, 8, 0, None, 0, None, None, None, None, None) == INVALID
    assert b"NULL" in err()
    assert lib.pnr_mesh_distance_reduce(None, None, 4, None, None, 4, None, None, 0.01, None, None) == INVALID
    assert b"NULL" in err()
    # refused shapes need no workspace; accepted ones always some
    assert lib.pnr_nearest_workspace_bytes(0, 5) == 0 and lib.pnr_nearest_workspace_bytes(5, 0) == 0
    assert lib.pnr_nearest_workspace_bytes(2 ** 31, 5) == 0 and b"2^31" in err()
    assert lib.pnr_nearest_workspace_bytes(5, 65535 * 4096 + 1) == 0
    assert lib.pnr_nearest_workspace_bytes(5, 5) > 0
    from pnr import ops

    S = ops.NEAREST_SLICE
    assert lib.pnr_nearest_workspace_bytes(1000, 2 * S + 1) >= 3 * 1000 * 8
    assert lib.pnr_mesh_sample_workspace_bytes(0) == 0 and lib.pnr_mesh_sample_workspace_bytes(2 ** 31) == 0
    assert lib.pnr_mesh_sample_workspace_bytes(1000) >= 8000
    assert lib.pnr_abi_version() == 8


def test_python_constants_are_the_headers():
    import re

    from pnr import ops

    text = open(os.path.join(REPO, "include", "pnr_abi.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PNR_[A-Z_]+) (\d+)", text)}
    assert (ops.NEAREST_QUERIES, ops.NEAREST_TILE, ops.NEAREST_SLICE, ops.MESH_SCAN_CHUNK, _lib.RNG_MESH) == (
        defs["PNR_NEAREST_QUERIES"], defs["PNR_NEAREST_TILE"], defs["PNR_NEAREST_SLICE"], defs["PNR_MESH_SCAN_CHUNK"],
        defs["PNR_RNG_MESH"])
    assert ops.NEAREST_SLICE % ops.NEAREST_TILE == 0 and evaluate._RNG_MESH == mesh_ref.RNG_MESH == _lib.RNG_MESH
    assert tuple(ops.MESH_DISTANCE_KEYS) == tuple(evaluate.MESH_METRIC_NAMES)


def test_host_draws_are_the_oracle_stream():
    for seed in (0, 7, 2 ** 40 + 3):
        assert np.array_equal(evaluate._draws(seed, evaluate._RNG_MESH, 1001),
                              philox.stream(seed, 0, mesh_ref.RNG_MESH, 1001, 3))


def test_host_sampling_is_the_restatement():
    v, f = mesh_ref.icosphere(2, 1.3)
    f = f.copy()
    f[::5] = f[::5, :1]                       # every fifth face collapsed to a point
    p, nrm, tri, total = evaluate.sample_mesh_np(v, f, 3000, seed=11)
    ref = mesh_ref.sample(v, f, 3000, 11)
    assert np.array_equal(tri, ref["tri"]) and total == ref["total"]
    assert (ref["area"][tri] > 0).all()
    assert np.abs(p - ref["points"]).max() <= 8 * mesh_ref.U * np.abs(v).max()
    assert np.abs(nrm - ref["normals"]).max() < 1e-6
    # on the sphere's faces: inside the sphere, outside the inscribed one
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    sag, _ = mesh_ref.sphere_slack(2, 1.3, 1)
    assert r.max() <= 1.3 * (1 + 1e-6) and r.min() >= 1.3 - sag - 1e-6


def test_numpy_backend_on_concentric_spheres():
    n = 20000
    inner, outer = mesh_ref.icosphere(3, 1.0), mesh_ref.icosphere(3, 1.1)
    sag_in, _ = mesh_ref.sphere_slack(3, 1.0, n)
    sag_out, spacing = mesh_ref.sphere_slack(3, 1.1, n)
    s = max(sag_in, sag_out) + spacing
    assert s < 0.05, s
    m = evaluate.mesh_metrics(inner, outer, n_samples=n, tau=0.2, seed=3, backend="numpy")
    print(m, "s =", s)
    assert set(m) == set(evaluate.MESH_METRIC_NAMES)
    for k in ("accuracy", "completeness", "chamfer_l1"):
        assert 0.1 - s <= m[k] <= 0.1 + s, (k, m[k], s)
    assert (0.1 - s) ** 2 <= m["chamfer_l2"] <= (0.1 + s) ** 2
    assert m["precision"] == m["recall"] == m["fscore"] == 1.0       # every distance is below 0.1 + s < tau
    assert m["normal_consistency"] > 0.99                            # concentric: parallel normals
    tight = evaluate.mesh_metrics(inner, outer, n_samples=2000, tau=0.05, seed=3, backend="numpy")
    assert tight["precision"] == tight["recall"] == tight["fscore"] == 0.0   # and none below 0.1 - s > tau


def test_empty_prediction_is_a_result():
    gt = mesh_ref.icosphere(1)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    for backend in ("numpy", "auto"):
        m = evaluate.mesh_metrics(empty, gt, n_samples=100, backend=backend)
        for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2"):
            assert m[k] == float("inf")
        for k in ("precision", "recall", "fscore", "normals_accuracy", "normals_completeness", "normal_consistency"):
            assert m[k] == 0.0
    with pytest.raises(ValueError):
        evaluate.mesh_metrics(gt, empty, n_samples=100, backend="numpy")


def test_stl_indexed_round_trip(tmp_path):
    v, f = mesh_ref.icosphere(1, 0.7)
    path = str(tmp_path / "s.stl")
    mesh.write_stl(path, v, f)
    rv, rf = mesh.read_stl_indexed(path)
    assert rv.dtype == np.float32 and rf.dtype == np.int32
    assert rf.shape == f.shape and np.array_equal(rf, np.arange(3 * len(f)).reshape(-1, 3))
    assert np.array_equal(rv[rf], v[f])
    mesh.write_stl(path, rv, rf)
    assert np.array_equal(mesh.read_stl_indexed(path)[0], rv)
    mesh.write_stl(path, v[:0], f[:0])
    ev, ef = mesh.read_stl_indexed(path)
    assert ev.shape == (0, 3) and ef.shape == (0, 3)


def test_normalize_bounds_on_a_known_box():
    import torch

    box = np.array([[1, 2, 3], [5, 2, 3], [1, 4, 3], [1, 2, 9], [5, 4, 9]], np.float32)   # centre (3, 3, 6)
    out = mesh.normalize_bounds(box, 2.0)
    half = np.array([2.0, 1.0, 3.0])
    want = (box - np.array([3, 3, 6])) * 2.0 / np.linalg.norm(half)
    assert out.dtype == np.float32 and np.allclose(out, want, atol=1e-6)
    assert abs(np.linalg.norm(out, axis=1).max() - 2.0) < 1e-6
    t = mesh.normalize_bounds(torch.from_numpy(box), 2.0)
    assert torch.is_tensor(t) and np.allclose(t.numpy(), want, atol=1e-6)
    assert mesh.normalize_bounds(box[:0]).shape == (0, 3)


def test_eval_mesh_script_numpy_backend(tmp_path):
    """Three synthetic objects, one without ground truth: predicted spheres of radius 0.5 and 0.4 in
    the grid's world cube, ground truths brought to radius 0.55 (--normalize gt), so the distances
    are the gaps 0.05 and 0.15 up to the tessellation and the sample spacing."""
    n, res = 4000, 33
    out, gt = mesh_ref.write_eval_tree(str(tmp_path), res, {"a": (0.5, 3.0), "b": (0.4, 1.0), "c": (0.5, None)})
    cmd = [sys.executable, os.path.join(REPO, "scripts", "eval_mesh.py"), "-O", out, "-G", gt, "--mesh_res", str(res),
           "--normalize", "gt", "--gt_radius", "0.55", "--n_samples", str(n), "--tau", "0.1", "--seed", "5",
           "--metrics_backend", "numpy"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr.count("skipped") == 1 and "c.stl" in r.stderr
    assert not os.path.exists(os.path.join(out, "c", "mesh_metrics.txt"))
    rows = {k: _read(os.path.join(out, k, "mesh_metrics.txt")) for k in ("a", "b")}
    sag, spacing = mesh_ref.sphere_slack(3, 0.55, n)
    s = sag + spacing + 2.0 / (res - 1) * 2.0 ** -20    # and the fp32 index units of the written STL
    for k, gap in (("a", 0.05), ("b", 0.15)):
        assert list(rows[k]) == list(evaluate.MESH_METRIC_NAMES)
        assert gap - s <= rows[k]["accuracy"] <= gap + s and gap - s <= rows[k]["completeness"] <= gap + s
    assert rows["a"]["fscore"] == 1.0 and rows["b"]["fscore"] == 0.0      # 0.05 + s < tau = 0.1 < 0.15 - s
    allm = open(os.path.join(out, "all_mesh_metrics.txt")).read().split("\n")
    assert allm[-2] == "objects 2" and allm[-1] == ""
    means = {k: float(x) for k, x in (ln.split() for ln in allm[:-2])}
    for k in evaluate.MESH_METRIC_NAMES:
        assert means[k] == (0.0 + rows["a"][k] + rows["b"][k]) / 2
    # a second run keeps the files (no --overwrite) and reduces again
    before = os.path.getmtime(os.path.join(out, "a", "mesh_metrics.txt"))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ">>> SCORED 0 OBJECTS" in r.stdout
    assert os.path.getmtime(os.path.join(out, "a", "mesh_metrics.txt")) == before
