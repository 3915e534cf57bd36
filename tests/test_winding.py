"""Host side of the mesh containment (no GPU): the refusals of the three ABI entries through the
ctypes binding, the constants, the host restatement of the PNR_RNG_VOLUME draws, winding_np against
tests/winding_ref.py, pnr.evaluate.volume_iou on its numpy backend and scripts/eval_mesh.py --iou end
to end.  The device kernels are tests/test_gpu_winding.py's."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mc_ref
import mesh_ref
from mesh_ref import _lines
import winding_ref
from oracle import philox
from pnr import _lib, evaluate, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def test_abi_entries_refuse_empty_and_null_arguments():
    lib = _lib.load()
    err = lib.pnr_last_error
    # sizes of 0
    assert lib.pnr_winding(None, 0, None, 0, None, 0, None, 0, None, None) == INVALID and b"pnr_winding" in err()
    assert lib.pnr_box_sample(None, None, 0, 0, None, None) == INVALID and b"pnr_box_sample" in err()
    # NULL required pointers at valid sizes
    assert lib.pnr_winding(None, 3, None, 1, None, 8, None, 0, None, None) == INVALID
    assert b"pnr_winding" in err() and b"NULL" in err()
    assert lib.pnr_box_sample(None, None, 8, 0, None, None) == INVALID
    assert b"pnr_box_sample" in err() and b"NULL" in err()
    # bounds are checked on the host before anything is launched; `points` is never written here
    box = lambda *v: ctypes.cast((ctypes.c_float * 3)(*v), ctypes.c_void_p)   # noqa: E731
    dummy = ctypes.c_void_p(256)
    for lo, hi in (((0, 0, 0), (1, -1, 1)), ((0, 0, 0), (1, float("inf"), 1)), ((float("nan"), 0, 0), (1, 1, 1))):
        lo_a, hi_a = box(*lo), box(*hi)
        assert lib.pnr_box_sample(lo_a, hi_a, 8, 0, dummy, None) == INVALID
        assert b"pnr_box_sample" in err() and b"bounds" in err()
    # refused shapes need no workspace; accepted ones always some
    wb = lib.pnr_winding_workspace_bytes
    assert wb(0, 5) == 0 and b"pnr_winding" in err()
    assert wb(5, 0) == 0 and wb(2 ** 31, 5) == 0 and wb(5, 2 ** 31) == 0
    assert wb(5, 65535 * ops.WINDING_SLICE + 1) == 0 and b"pnr_winding" in err()
    assert wb(5, 5) > 0 and wb(2 ** 31 - 1, ops.WINDING_SLICE) > 0
    assert wb(1000, 2 * ops.WINDING_SLICE + 1) >= 3 * 1000 * 8
    assert lib.pnr_abi_version() == 8


def test_python_constants_are_the_headers():
    text = open(os.path.join(REPO, "include", "pnr_abi.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PNR_[A-Z_]+) (\d+)", text)}
    assert (ops.WINDING_QUERIES, ops.WINDING_TILE, ops.WINDING_SLICE, _lib.RNG_VOLUME) == (
        defs["PNR_WINDING_QUERIES"], defs["PNR_WINDING_TILE"], defs["PNR_WINDING_SLICE"], defs["PNR_RNG_VOLUME"])
    assert ops.WINDING_SLICE % ops.WINDING_TILE == 0
    assert _lib.RNG_VOLUME == 5 == evaluate._RNG_VOLUME
    assert tuple(evaluate.VOLUME_METRIC_NAMES) == ("iou", "volume_pred", "volume_gt", "n_points")


def test_host_draws_are_the_oracle_stream():
    for seed in (0, 7, 2 ** 40 + 3):
        assert np.array_equal(evaluate._draws(seed, evaluate._RNG_VOLUME, 1001),
                              philox.stream(seed, 0, 5, 1001, 3))


def test_host_box_samples_lie_in_the_box():
    lo, hi = np.array([-1.5, 2.0, 36.0], np.float32), np.array([0.25, 2.0, 38.5], np.float32)
    p = evaluate.box_sample_np(lo, hi, 5000, seed=3)
    assert p.dtype == np.float32 and p.shape == (5000, 3)
    assert (p >= lo).all() and (p <= hi).all() and (p[:, 1] == 2.0).all()
    assert np.array_equal(p[:100], evaluate.box_sample_np(lo, hi, 100, seed=3))
    u = philox.stream(3, 0, 5, 5000, 3).astype(np.float64)
    assert np.abs(p - (lo + u * (hi.astype(np.float64) - lo))).max() <= 2.0 ** -24 * 38.5


def test_host_winding_number_on_a_sphere():
    v, f = mesh_ref.icosphere(2)
    rng = np.random.default_rng(40)
    d = rng.standard_normal((400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # the inscribed sphere touches the faces at their nearest point to the centre
    fv = v.astype(np.float64)[f]
    nrm = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0])
    inscribed = float(np.abs((fv[:, 0] * nrm).sum(1) / np.linalg.norm(nrm, axis=1)).min())
    assert 0.9 < inscribed < 1.0
    inside = (d[:200] * rng.uniform(0, 0.9 * inscribed, (200, 1))).astype(np.float32)
    outside = (d[200:] * rng.uniform(1.01, 3.0, (200, 1))).astype(np.float32)
    box = rng.uniform(-1.25, 1.25, (500, 3)).astype(np.float32)
    for pts in (inside, outside, box):
        assert np.abs(evaluate.winding_np(v, f, pts) - winding_ref.winding64(v, f, pts)).max() <= 1e-12
        assert np.abs(evaluate.winding_np(v, f, pts, chunk=7) - winding_ref.winding64(v, f, pts)).max() <= 1e-12
    assert np.abs(evaluate.winding_np(v, f, inside) - 1.0).max() <= 1e-9
    assert np.abs(evaluate.winding_np(v, f, outside)).max() <= 1e-9
    # inward faces: -1 inside
    assert np.abs(evaluate.winding_np(v, f[:, ::-1], inside) + 1.0).max() <= 1e-9
    # a query on a vertex is finite, a face with a bad index contributes nothing
    on = evaluate.winding_np(v, f, v[:50])
    assert np.isfinite(on).all() and on.min() >= -1e-9 and on.max() <= 1 + 1e-9
    bad = np.concatenate([f, [[0, 1, len(v)], [-1, 2, 3]]]).astype(np.int32)
    assert np.array_equal(evaluate.winding_np(v, bad, box), evaluate.winding_np(v, f, box))


def test_fp32_emulation_stays_within_the_device_bound():
    """winding32 (the device's arithmetic up to atan2f) against winding64 on a translated sphere: the
    measured error the GPU tests' bound of 1e-6 rests on."""
    v, f = mesh_ref.icosphere(3)
    v = v + np.array([37, -5, 11], np.float32)
    rng = np.random.default_rng(41)
    pts = np.concatenate([rng.uniform(-1.25, 1.25, (600, 3)).astype(np.float32) + np.array([37, -5, 11], np.float32),
                          winding_ref.near_sphere([37, -5, 11], 1.0, 100, 1e-3, rng), v[:50]])
    e = np.abs(winding_ref.winding32(v, f, pts) - winding_ref.winding64(v, f, pts)).max()
    print("max |winding32 - winding64| = %.3g" % e)
    assert e <= 1e-6


_IOU = {}


def sphere_iou():
    if not _IOU:
        _IOU["r"] = evaluate.volume_iou(mesh_ref.icosphere(3, 0.8), mesh_ref.icosphere(3, 1.0), n_points=20000,
                                        backend="numpy")
    return _IOU["r"]


def test_volume_iou_numpy_backend_on_concentric_spheres():
    """Two similar concentric polyhedra: the true IoU is exactly 0.8^3 = 0.512.  About 8,900 of the
    20,000 points fall in the union, so sigma = sqrt(0.512 * 0.488 / 8900) = 0.0053."""
    r = sphere_iou()
    print(r)
    assert list(r) == list(evaluate.VOLUME_METRIC_NAMES) and all(type(x) is float for x in r.values())
    assert abs(r["iou"] - 0.512) <= 0.027
    vol = mc_ref.signed_volume(*mesh_ref.icosphere(3, 1.0))
    assert abs(r["volume_gt"] - vol) <= 0.05 * vol
    assert abs(r["volume_pred"] - 0.512 * vol) <= 0.05 * vol
    assert r["n_points"] == 20000.0


def test_volume_iou_of_an_inside_out_ground_truth():
    v, f = mesh_ref.icosphere(3, 1.0)
    assert mc_ref.signed_volume(v, f[:, ::-1]) < 0
    r = evaluate.volume_iou(mesh_ref.icosphere(3, 0.8), (v, np.ascontiguousarray(f[:, ::-1])), n_points=20000,
                            backend="numpy")
    assert r == sphere_iou()


def test_empty_prediction_is_a_result():
    gt = mesh_ref.icosphere(1)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    r = evaluate.volume_iou(empty, gt, n_points=500, backend="numpy")
    assert r["iou"] == 0.0 and r["volume_pred"] == 0.0 and r["volume_gt"] > 0 and r["n_points"] == 500.0
    with pytest.raises(ValueError):
        evaluate.volume_iou(gt, empty, n_points=500, backend="numpy")
    with pytest.raises(ValueError):
        evaluate.volume_iou(gt, gt, n_points=500, backend="cuda")


def test_eval_mesh_script_iou_numpy_backend(tmp_path):
    """Predicted spheres of radius 0.5 and 0.4 in the grid's world cube against ground truths brought
    to radius 0.55 (--normalize gt): concentric, so the IoU is (r / 0.55)^3 up to the sampling error
    (about 1,100 of 3,000 points in the union: sigma 0.015, 5 sigma < 0.1).  Then the same tree without --iou: the
    files are those lines without the volume ones, the parent's format."""
    n, res = 1500, 33
    out, gt = mesh_ref.write_eval_tree(str(tmp_path), res, {"a": (0.5, 3.0), "b": (0.4, 1.0), "c": (0.5, None)})
    cmd = [sys.executable, os.path.join(REPO, "scripts", "eval_mesh.py"), "-O", out, "-G", gt, "--mesh_res", str(res),
           "--normalize", "gt", "--gt_radius", "0.55", "--n_samples", str(n), "--tau", "0.1", "--seed", "5",
           "--metrics_backend", "numpy"]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-3000:]
    old = {k: open(os.path.join(out, k, "mesh_metrics.txt")).read() for k in ("a", "b")}
    old_all = open(os.path.join(out, "all_mesh_metrics.txt")).read()
    for k in ("a", "b"):
        rows = _lines(os.path.join(out, k, "mesh_metrics.txt"))
        assert [r[0] for r in rows] == list(evaluate.MESH_METRIC_NAMES)
        assert old[k] == "".join("{} {!r}\n".format(name, float(val)) for name, val in rows)
    assert [r[0] for r in _lines(os.path.join(out, "all_mesh_metrics.txt"))] == list(evaluate.MESH_METRIC_NAMES) + [
        "objects"]
    # --iou on files written without it: the reduce names the object and stops
    r = subprocess.run(cmd + ["--iou", "-R"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "object a" in r.stderr
    assert open(os.path.join(out, "all_mesh_metrics.txt")).read() == old_all
    r = subprocess.run(cmd + ["--iou", "--n_iou_points", "3000", "--overwrite"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    names = list(evaluate.MESH_METRIC_NAMES) + list(evaluate.VOLUME_METRIC_NAMES)
    vals = {}
    for k, radius in (("a", 0.5), ("b", 0.4)):
        text = open(os.path.join(out, k, "mesh_metrics.txt")).read()
        assert text.startswith(old[k])                       # the old lines unchanged, then the new ones
        rows = _lines(os.path.join(out, k, "mesh_metrics.txt"))
        assert [r[0] for r in rows] == names
        vals[k] = {r[0]: float(r[1]) for r in rows}
        assert abs(vals[k]["iou"] - (radius / 0.55) ** 3) <= 0.1
        assert vals[k]["n_points"] == 3000.0
    rows = _lines(os.path.join(out, "all_mesh_metrics.txt"))
    assert [r[0] for r in rows] == names + ["objects"] and rows[-1][1] == "2"
    for name, val in rows[:-1]:
        assert float(val) == (0.0 + vals["a"][name] + vals["b"][name]) / 2
    # and without --iou again: byte for byte the first run's files
    r = subprocess.run(cmd + ["--overwrite"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert {k: open(os.path.join(out, k, "mesh_metrics.txt")).read() for k in ("a", "b")} == old
    assert open(os.path.join(out, "all_mesh_metrics.txt")).read() == old_all
