"""Host side of the mesh rendering (no GPU): the new ABI entries through the ctypes binding and their
refusals, the PNR_RASTER_* mirrors, pnr.evaluate.raycast_np against tests/raster_ref.py, the golden-spiral
cameras, the supersampling camera, scripts/render_meshes.py on its numpy backend and the --sil_views flags of
scripts/eval_mesh.py.  The device kernels are tests/test_gpu_mesh_raster.py's."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ref
from mesh_ref import _lines
import raster_ref as R
from pnr import _lib, evaluate, mesh, ops
from pnr.data import SRNDataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NEW = ("pnr_mesh_raster_workspace_bytes", "pnr_mesh_raster", "pnr_mesh_raster_set_small", "pnr_mesh_shade")


def test_library_exports_the_new_symbols_at_abi_8():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert _lib.load().pnr_abi_version() == 8 == _lib.ABI_VERSION
    header = open(os.path.join(REPO, "include", "pnr_abi.h")).read()
    assert "Mesh rendering" in header and all(re.search(r"\b%s\s*\(" % n, header) for n in NEW)


def test_python_constants_are_the_headers():
    text = open(os.path.join(REPO, "include", "pnr_abi.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PNR_[A-Z_]+) (\d+)", text)}
    assert (ops.RASTER_BLOCK, ops.RASTER_TILE, ops.RASTER_SMALL_PIXELS, ops.RASTER_MAX_LIGHTS) == (
        defs["PNR_RASTER_BLOCK"], defs["PNR_RASTER_TILE"], defs["PNR_RASTER_SMALL_PIXELS"], defs["PNR_RASTER_MAX_LIGHTS"])
    assert ops.RASTER_TILE ** 2 == 64 and ops.RASTER_BLOCK % 64 == 0
    assert tuple(evaluate.SIL_METRIC_NAMES) == ("sil_iou", "sil_depth_l1", "sil_views")


def test_abi_entries_refuse_bad_shapes_and_null_arguments():
    lib = _lib.load()
    err = lib.pnr_last_error
    wb = lib.pnr_mesh_raster_workspace_bytes
    assert wb(1, 1, 1, 1) >= 8 and wb(128, 128, 128, 165000) >= 128 * 128 * 128 * 8
    assert wb(1, 8192, 8192, 2 ** 31 - 1) >= 8192 * 8192 * 8
    for nv, h, w, t in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 0), (1, 8193, 8, 1), (1, 8, 8193, 1),
                        (1, 8, 8, 2 ** 31), (2 ** 31, 1, 1, 1), (32, 8192, 8192, 1)):
        assert wb(nv, h, w, t) == 0, (nv, h, w, t)
    d = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on the host
    assert lib.pnr_mesh_raster(None, 0, None, 0, None, 0, 4, 0, 0, 1.0, 1.0, 0.0, 0.0, None, 0, None, None, None) == INVALID
    assert b"pnr_mesh_raster" in err()
    assert lib.pnr_mesh_raster(None, 3, None, 1, None, 1, 4, 8, 8, 1.0, 1.0, 0.0, 0.0, None, 0, None, None, None) == INVALID
    assert b"NULL" in err()
    assert lib.pnr_mesh_raster(d, 3, d, 1, d, 1, 5, 8, 8, 1.0, 1.0, 0.0, 0.0, d, 512, d, d, None) == INVALID
    assert b"pose_rows" in err()
    assert lib.pnr_mesh_raster(d, 3, d, 1, d, 1, 4, 8193, 8, 1.0, 1.0, 0.0, 0.0, d, 512, d, d, None) == UNSUPPORTED
    assert lib.pnr_mesh_raster(d, 3, d, 1, d, 1, 4, 8, 8, 0.0, 1.0, 0.0, 0.0, d, 512, d, d, None) == INVALID
    assert b"fx" in err()
    assert lib.pnr_mesh_raster(d, 3, d, 1, d, 1, 4, 8, 8, 1.0, float("nan"), 0.0, 0.0, d, 512, d, d, None) == INVALID
    assert lib.pnr_mesh_raster(d, 3, d, 1, d, 1, 4, 8, 8, 1.0, 1.0, 0.0, 0.0, d, 8, d, d, None) != 0
    assert b"workspace" in err()
    assert lib.pnr_mesh_shade(None, 3, None, 1, None, 1, 4, 8, 8, 1.0, 1.0, 0.0, 0.0, None, None, None, None, 0, None,
                              0.0, None, None, None, None) == INVALID and b"pnr_mesh_shade" in err()
    assert lib.pnr_mesh_shade(d, 3, d, 1, d, 1, 4, 8, 8, 1.0, 1.0, 0.0, 0.0, d, d, d, d, 9, d, 0.0, d, d, None,
                              None) == INVALID and b"n_lights" in err()
    # the threshold knob returns the previous value and restores the default
    assert lib.pnr_mesh_raster_set_small(5) == ops.RASTER_SMALL_PIXELS
    assert lib.pnr_mesh_raster_set_small(-1) == 5 and lib.pnr_mesh_raster_set_small(-1) == ops.RASTER_SMALL_PIXELS
    # the wrappers refuse host tensors: no CPU fallback
    v, f = R.box_mesh()
    with pytest.raises(ValueError, match="HIP device"):
        ops.mesh_raster(torch.from_numpy(v), torch.from_numpy(f), torch.eye(4)[None], 8, 8, 8.0)


def test_raycast_np_equals_the_reference_on_case_a():
    k = R.case("A")
    face, depth = evaluate.raycast_np(k["v"], k["f"], k["poses"], k["size"], k["size"], k["focal"], k["c"])
    assert face.dtype == np.int32 and depth.dtype == np.float64 and face.shape == k["face64"].shape
    m = k["sure"]
    assert np.array_equal(face >= 0, k["face64"] >= 0)            # fp64 both: also on the unsure pixels here
    assert np.array_equal(face[m], k["face64"][m])
    assert np.abs(depth - k["depth64"])[m].max() <= 1e-12
    assert (depth[face < 0] == 0).all()
    # the same rules for bad input, (NV, 3, 4) poses and chunking
    v_bad = np.concatenate([k["v"], [[np.nan, 0, 0]]]).astype(np.float32)
    bad = np.array([[0, 1, len(v_bad)], [0, 1, len(k["v"])], [2, 2, 5], [-1, 0, 1]], np.int32)
    poses = k["poses"][:2].copy()
    poses[1, 2, 3] = np.nan
    got = evaluate.raycast_np(v_bad, np.concatenate([bad, k["f"]]), poses[:, :3], k["size"], k["size"], k["focal"],
                              k["c"], chunk=77)
    assert np.array_equal(got[0][0], np.where(face[0] >= 0, face[0] + len(bad), -1))
    assert np.array_equal(got[1][0], depth[0]) and (got[0][1] == -1).all() and (got[1][1] == 0).all()
    # exact tilings: the lowest face among those that contain the ray
    for step, soup in ((1, False), (4, True)):
        v, f = R.plane_quads(step, soup=soup)
        got = evaluate.raycast_np(v, f, np.eye(4, dtype=np.float32)[None], 17, 17, 16.0, 8.0)
        assert np.array_equal(got[0][0], R.lowest_containing_face(v, f, 17, 17, 16.0, 16.0, 8.0, 8.0))


def test_sphere_poses_are_the_golden_spiral():
    for n, radius in ((1, 2.0), (7, 1.3), (128, 1.3)):
        poses, file_poses = evaluate.sphere_poses(n, radius)
        assert poses.shape == file_poses.shape == (n, 4, 4) and poses.dtype == np.float64
        assert np.abs(poses - R.golden_poses(n, radius).astype(np.float64)).max() <= 1e-6
        assert np.array_equal(file_poses @ np.diag([1.0, -1.0, -1.0, 1.0]), poses)       # what the loader applies
        assert np.allclose(np.linalg.norm(poses[:, :3, 3], axis=1), radius) and (poses[:, 2, 3] > 0).all()
        # each camera looks at the origin down its -z axis, x stays horizontal
        assert np.allclose(-poses[:, :3, 2] * radius, -poses[:, :3, 3]) and np.allclose(poses[:, 2, 0], 0.0)
        assert np.allclose(np.einsum("nij,nkj->nik", poses[:, :3, :3], poses[:, :3, :3]), np.eye(3), atol=1e-12)
        assert np.allclose(np.linalg.det(poses[:, :3, :3]), 1.0)
    full, _ = evaluate.sphere_poses(8, 1.0, hemisphere=False)
    assert (full[:4, 2, 3] > 0).all() and (full[4:, 2, 3] < 0).all()
    upper, _ = evaluate.sphere_poses(4, 1.0)
    assert np.allclose(upper, full[:4])
    with pytest.raises(ValueError):
        evaluate.sphere_poses(0, 1.0)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_ssaa_samples_are_centred_on_the_pixel_ray(k):
    fx, fy, cx, cy = 37.0, 29.5, 17.25, 14.5
    fxk, fyk, cxk, cyk = evaluate.ssaa_camera(k, fx, fy, cx, cy)
    for i, j in ((0, 0), (5, 11), (39, 23)):
        sub_i, sub_j = np.arange(k * i, k * i + k), np.arange(k * j, k * j + k)
        assert abs(((sub_i - cxk) / fxk).mean() - (i - cx) / fx) <= 1e-12
        assert abs(((sub_j - cyk) / fyk).mean() - (j - cy) / fy) <= 1e-12


def test_render_mesh_views_numpy_backend():
    v, f = mesh_ref.icosphere(1, 0.5)
    poses, _ = evaluate.sphere_poses(3, 1.3)
    poses = torch.from_numpy(poses).float()
    kw = dict(lights=[(1.3, 1.3, 1.3)], weights=[0.7], albedo=(0.8, 0.6, 0.4), ambient=0.2)
    one = evaluate.render_mesh_views(v, f, poses, 16, 16, 16.4, backend="numpy", **kw)
    two = evaluate.render_mesh_views(v, f, poses, 16, 16, 16.4, ssaa=2, backend="numpy", **kw)
    assert one["rgb"].shape == two["rgb"].shape == (3, 16, 16, 3) and two["face"].shape == (3, 32, 32)
    assert set(np.unique(one["mask"].numpy())) == {0.0, 1.0}
    assert set(np.unique(two["mask"].numpy())) <= {0.0, 0.25, 0.5, 0.75, 1.0} and 0.25 in two["mask"]
    face, depth = R.cast64(v, f, poses.numpy(), 16, 16, 16.4)
    assert np.array_equal(one["face"].numpy(), face) and np.abs(one["depth"].numpy() - depth).max() <= 1e-6
    # the box average: each pixel is the mean of its 2 x 2 samples
    hi_face, hi_depth = two["face"].numpy(), two["depth"].numpy()
    cam = evaluate.ssaa_camera(2, 16.4, 16.4, 8.0, 8.0)
    hi_rgb, _ = evaluate.shade_np(v, f, poses, 32, 32, cam[:2], hi_face, hi_depth, c=cam[2:], **kw)
    want = hi_rgb.reshape(3, 16, 2, 16, 2, 3).mean((2, 4))
    assert np.abs(two["rgb"].numpy() - want).max() <= 1e-6
    assert (one["rgb"].numpy()[face < 0] == 1.0).all() and one["rgb"].numpy()[face >= 0].max() <= 254.0 / 255.0 + 1e-7
    with pytest.raises(ValueError):
        evaluate.render_mesh_views(v, f, poses, 16, 16, 16.4, backend="cuda")
    with pytest.raises(ValueError):
        evaluate.render_mesh_views(v, f, poses, 16, 16, 16.4, ssaa=0, backend="numpy")


def test_silhouette_scores_numpy_backend():
    v, f = mesh_ref.icosphere(1, 0.45)
    poses = R.golden_poses(3, 1.3)
    assert evaluate.silhouette_scores((v, f), (v, f), poses, 24, 24, 24.6, backend="numpy") == {
        "sil_iou": 1.0, "sil_depth_l1": 0.0, "sil_views": 3.0}
    small = (0.8 * v).astype(np.float32)
    got = evaluate.silhouette_scores((small, f), (v, f), poses, 24, 24, 24.6, backend="numpy")
    fa, da = R.cast64(small, f, poses, 24, 24, 24.6)
    fb, db = R.cast64(v, f, poses, 24, 24, 24.6)
    a, b = fa >= 0, fb >= 0
    assert abs(got["sil_iou"] - np.mean([(a[n] & b[n]).sum() / (a[n] | b[n]).sum() for n in range(3)])) <= 1e-12
    assert abs(got["sil_depth_l1"] - np.abs(da - db)[a & b].mean()) <= 1e-9
    away = poses.copy()
    away[:, :3, 2] *= -1
    away[:, :3, 0] *= -1
    assert evaluate.silhouette_scores((v, f), (v, f), away, 8, 8, 8.2, backend="numpy") == {
        "sil_iou": 1.0, "sil_depth_l1": float("inf"), "sil_views": 3.0}      # both empty in every view
    with pytest.raises(ValueError):
        evaluate.silhouette_scores((v, f), (v[:0], f[:0]), poses, 8, 8, 8.2, backend="numpy")


def test_render_meshes_script_numpy_backend(tmp_path):
    meshes, out = tmp_path / "stl", tmp_path / "pollen"
    meshes.mkdir()
    v, f = mesh_ref.icosphere(1, 3.0)
    mesh.write_stl(str(meshes / "ball.stl"), v + np.float32(5.0), f)        # off-centre and large: normalised away
    cmd = [sys.executable, os.path.join(REPO, "scripts", "render_meshes.py"), "-M", str(meshes), "-D", str(out),
           "--views", "10", "--size", "16", "--focal", "16.40625", "--backend", "numpy"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    gl, file_poses = evaluate.sphere_poses(10, 1.3)
    views = {"val": [0], "test": [9], "train": list(range(1, 9))}
    radius = 0.95 * 1.3 * np.sin(np.arctan(8.0 / 16.40625))
    sv, sf = mesh.read_stl_indexed(str(meshes / "ball.stl"))
    sv = mesh.normalize_bounds(sv, radius)
    assert abs(np.linalg.norm(sv, axis=1).max() - radius) <= 1e-6
    cam = evaluate.ssaa_camera(2, 16.40625, 16.40625, 8.0, 8.0)
    for stage, idx in views.items():
        dset = SRNDataset(str(out), stage=stage, image_size=(16, 16))
        assert len(dset) == 1
        item = dset[0]
        assert item["images"].shape == (len(idx), 3, 16, 16) and float(item["focal"]) == np.float32(16.40625)
        assert item["c"].tolist() == [8.0, 8.0]
        assert np.array_equal(item["poses"].numpy(), gl[idx].astype(np.float32))
        obj = item["path"]
        assert open(os.path.join(obj, "intrinsics.txt")).read() == (
            "16.406250 8.000000 8.000000 0.\n0. 16.406250 8.000000 0.\n0. 0. 1.\n16 16")
        near, far = (float(t) for t in open(os.path.join(obj, "near_far.txt")).read().split())
        assert abs(near - (1.3 - radius)) <= 1e-6 and abs(far - (1.3 + radius)) <= 1e-6
        text = open(os.path.join(obj, "pose", "000000.txt")).read()
        assert text == "".join(" ".join("%.16f" % x for x in row) + "\n" for row in file_poses[idx[0]])
        # the default --ssaa 2: a pixel is foreground unless it rounds to white; every fully covered one is not
        face, _ = evaluate.raycast_np(sv, sf, gl[idx].astype(np.float32), 32, 32, cam[:2], cam[2:])
        cover = (face >= 0).reshape(len(idx), 16, 2, 16, 2).mean((2, 4))
        fg = item["masks"][:, 0].numpy() > 0
        assert fg[cover == 1.0].all() and not fg[cover == 0.0].any() and (cover == 1.0).sum() > 20 * len(idx)
    # a second run skips the object; --overwrite renders it again, byte for byte
    png = os.path.join(str(out), "pollen_train", "ball", "rgb", "000003.png")
    before = open(png, "rb").read()
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "skipped" in run.stdout
    run = subprocess.run(cmd + ["--overwrite", "--write_depth"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and open(png, "rb").read() == before
    depth = np.load(os.path.join(str(out), "pollen_train", "ball", "depth", "000003.npy"))
    assert depth.shape == (16, 16) and depth.dtype == np.float32 and 0.3 < (depth > 0).mean() < 0.9


def test_eval_mesh_script_silhouette_flags(tmp_path):
    n, res = 800, 33
    out, gt = mesh_ref.write_eval_tree(str(tmp_path), res, {"a": (0.5, 3.0), "b": (0.4, 1.0)})
    cmd = [sys.executable, os.path.join(REPO, "scripts", "eval_mesh.py"), "-O", out, "-G", gt, "--mesh_res", str(res),
           "--n_samples", str(n), "--tau", "0.1", "--seed", "5", "--metrics_backend", "numpy"]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-3000:]
    # without --sil_views: the bytes the script wrote before, restated from the library's scores
    old = {}
    for k in ("a", "b"):
        pv, pf = mesh.read_stl_indexed(os.path.join(out, k, k + "_mesh.stl"))
        gv, gf = mesh.read_stl_indexed(os.path.join(gt, k + ".stl"))
        pv = mesh.normalize_bounds(pv * (2.0 / (res - 1)) - 1.0)
        scores = evaluate.mesh_metrics((pv, pf), (mesh.normalize_bounds(gv), gf), n_samples=n, tau=0.1, seed=5,
                                       backend="numpy")
        old[k] = open(os.path.join(out, k, "mesh_metrics.txt")).read()
        assert old[k] == "".join("{} {!r}\n".format(name, float(scores[name])) for name in evaluate.MESH_METRIC_NAMES)
    old_all = open(os.path.join(out, "all_mesh_metrics.txt")).read()
    assert [r[0] for r in _lines(os.path.join(out, "all_mesh_metrics.txt"))] == list(evaluate.MESH_METRIC_NAMES) + [
        "objects"]
    sil = ["--sil_views", "3", "--sil_size", "24", "--sil_focal", "24.6"]
    # files written without the flag: the reduce names the object and stops
    r = subprocess.run(cmd + sil + ["-R"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "object a" in r.stderr and "silhouette" in r.stderr
    assert open(os.path.join(out, "all_mesh_metrics.txt")).read() == old_all
    # one object rescored with the flag, the other not: still refused, by the other's name
    os.remove(os.path.join(out, "a", "mesh_metrics.txt"))
    r = subprocess.run(cmd + sil, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "object b" in r.stderr
    r = subprocess.run(cmd + sil + ["--overwrite"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    names = list(evaluate.MESH_METRIC_NAMES) + list(evaluate.SIL_METRIC_NAMES)
    vals = {}
    for k in ("a", "b"):
        text = open(os.path.join(out, k, "mesh_metrics.txt")).read()
        assert text.startswith(old[k])                          # the old lines unchanged, then the three new ones
        rows = _lines(os.path.join(out, k, "mesh_metrics.txt"))
        assert [r[0] for r in rows] == names
        vals[k] = {r[0]: float(r[1]) for r in rows}
        # a sphere against a sphere, both normalised to the unit sphere: nearly the same silhouette and depth
        assert vals[k]["sil_iou"] > 0.9 and vals[k]["sil_depth_l1"] < 0.05 and vals[k]["sil_views"] == 3.0
    rows = _lines(os.path.join(out, "all_mesh_metrics.txt"))
    assert [r[0] for r in rows] == names + ["objects"] and rows[-1][1] == "2"
    for name, val in rows[:-1]:
        assert float(val) == (0.0 + vals["a"][name] + vals["b"][name]) / 2
    # and without the flag again: byte for byte the first run's files
    r = subprocess.run(cmd + ["--overwrite"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert {k: open(os.path.join(out, k, "mesh_metrics.txt")).read() for k in ("a", "b")} == old
    assert open(os.path.join(out, "all_mesh_metrics.txt")).read() == old_all
    bad = subprocess.run(cmd + ["--sil_views", "-1"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--sil_views" in bad.stderr
