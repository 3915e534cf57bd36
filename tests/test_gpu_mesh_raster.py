"""Device tests of the mesh rendering (csrc/meshraster.hip; include/pnr_abi.h, "Mesh rendering") against
tests/raster_ref.py: the fp64 brute-force ray cast on the pixels it calls sure.

The depth bound.  raster_ref.raster32 emulates the kernel's fp32 per-(pixel, face) arithmetic on the host
(the same roundings and fmas).  Against the fp64 cast, on the sure pixels, its largest relative depth error
is 3.96e-7 in case A and 9.17e-7 in case B (measured on the host, no device involved).  DEPTH_RTOL is about
4 x the larger of the two: 3.7e-6, some 60 fp32 ulp.  Every test prints its own measured maximum.

The shading bound.  The colour is albedo x (ambient + sum of weights x cosines) and the normal a unit vector,
every term at most 1 in size.  evaluate_free_shade below writes the header's formula out in a chosen precision;
in fp32 against fp64, both on the same fp32 face and depth of case B (raster32's, on the host, no device
involved), it differs by at most 1.61e-7 in the colour and 8.03e-8 in the normal.  The bounds are 4 x that:
SHADE_ATOL = 6.4e-7 and NORMAL_ATOL = 3.2e-7.  test_shading evaluates both on the device's own face and depth
and prints the emulation's and the device's maxima."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ref
import raster_ref as R
from pnr import _lib, evaluate, mesh, ops, util
from pnr.data import SRNDataset

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_RTOL = 3.7e-6
SHADE_ATOL, NORMAL_ATOL = 6.4e-7, 3.2e-7


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dtype=dtype) if dtype is not None else t.cuda()


def raster(v, f, poses, w, h, focal, c=None):
    face, depth = ops.mesh_raster(dev(v, torch.float32), dev(f, torch.int32), dev(poses, torch.float32), w, h, focal, c)
    assert face.dtype == torch.int32 and depth.dtype == torch.float32
    assert tuple(face.shape) == tuple(depth.shape) == (len(poses), h, w)
    return face.cpu().numpy(), depth.cpu().numpy()


def check_against_reference(label, v, f, poses, w, h, focal, c=None, face64=None, depth64=None, sure=None):
    """hit / miss, depth and face of the device against the fp64 cast on the sure pixels; returns the
    device's (face, depth)."""
    if face64 is None:
        face64, depth64 = R.cast64(v, f, poses, w, h, focal, c)
        sure = R.sure(v, f, poses, w, h, focal, c, centre=(face64, depth64))
    face, depth = raster(v, f, poses, w, h, focal, c)
    assert ((face >= 0) == (face64 >= 0))[sure].all(), "%s: hit / miss differs on a sure pixel" % label
    assert (depth[face < 0] == 0).all() and (face >= -1).all() and (face < len(f)).all()
    hit = sure & (face64 >= 0)
    rel = np.abs(depth.astype(np.float64) - depth64)[hit] / depth64[hit] if hit.any() else np.zeros(1)
    print("%s: %d sure hits of %d pixels, max relative depth error %.3e (bound %.1e)"
          % (label, hit.sum(), hit.size, rel.max(), DEPTH_RTOL))
    assert rel.max() <= DEPTH_RTOL
    # the returned face is a valid answer: hit by that ray, and its t within the bound of the minimum
    inside, t = R.face_answers(v, f, poses, w, h, focal, face, c)
    assert inside[hit].all(), "%s: a returned face is not hit by its pixel's ray" % label
    assert (np.abs(t - depth64)[hit] <= DEPTH_RTOL * depth64[hit]).all()
    return face, depth


@pytest.mark.parametrize("name", ["A", "B"])
def test_parity_with_the_fp64_ray_cast(name):
    k = R.case(name)
    unsure, covered = 1.0 - k["sure"].mean(), (k["face64"] >= 0).mean()
    print("case %s: unsure %.4f, covered %.4f" % (name, unsure, covered))
    assert unsure <= 0.02 and 0.2 <= covered <= 0.8   # the test cannot hide behind its mask
    check_against_reference("case " + name, k["v"], k["f"], k["poses"], k["size"], k["size"], k["focal"], k["c"],
                            k["face64"], k["depth64"], k["sure"])


@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (8, 8), (9, 7), (65, 33)])
def test_image_sizes(w, h):
    v, f = R.sphere_with_floater(1)
    c = (0.0, 0.0) if w == 1 else None                # the single pixel's ray down the axis, at the sphere
    face, _ = check_against_reference("%d x %d" % (w, h), v, f, R.golden_poses(2, 1.3), w, h, 0.9 * max(w, h), c)
    assert (face >= 0).any()


def test_unequal_focals_and_off_centre():
    v, f = R.sphere_with_floater(2)
    check_against_reference("40 x 24", v, f, R.golden_poses(3, 1.3), 40, 24, (37.0, 29.5), (17.25, 14.5))


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, ops.RASTER_BLOCK + 1])
@pytest.mark.parametrize("nv", [1, 3])
def test_face_and_view_counts(n_faces, nv):
    v, f = R.sphere_with_floater(2)                      # 400 faces: the first n_faces of them
    check_against_reference("T = %d, NV = %d" % (n_faces, nv), v, f[:n_faces], R.golden_poses(nv, 1.3), 24, 24, 24.6)


@pytest.mark.parametrize("step,soup", [(1, False), (4, False), (1, True), (4, True)])
def test_rays_through_vertices_and_edges_are_exact(step, soup):
    """Every ray passes through a vertex (step 1) or through vertices and edges (step 4: bounds of 25 pixels and
    more, the wave path) of the tiling; every value is a short dyadic number, so fp32 and fp64 agree."""
    v, f = R.plane_quads(step, soup=soup)
    want = R.lowest_containing_face(v, f, 17, 17, 16.0, 16.0, 8.0, 8.0)
    assert (want >= 0).all()
    face, depth = raster(v, f, np.eye(4, dtype=np.float32)[None], 17, 17, 16.0, 8.0)
    assert (face[0] >= 0).all(), "a ray through a shared edge or vertex hit nothing"
    assert np.array_equal(face[0], want)
    X, Yn, length = R.pixel_dirs32(17, 17, 16.0, 16.0, 8.0, 8.0)
    assert np.array_equal(depth[0].reshape(-1), length)             # s = 1 exactly on the plane z = -1


def test_both_paths_give_the_same_bits():
    k = R.case("A")
    close = k["poses"].copy()
    close[:, :3, 3] *= 0.6                      # close up: faces of a hundred pixels and more
    poses = np.concatenate([k["poses"], close])
    base = raster(k["v"], k["f"], poses, 40, 40, 41.0)
    assert (base[0] >= 0).mean() > 0.2
    for small in (0, 4, 1 << 30):
        with ops.raster_small_pixels(small):
            got = raster(k["v"], k["f"], poses, 40, 40, 41.0)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.int32), base[1].view(np.int32)), small
    assert _lib.load().pnr_mesh_raster_set_small(-1) == ops.RASTER_SMALL_PIXELS


def test_large_faces():
    v, f = R.box_mesh(0.5)
    poses = R.golden_poses(2, 1.6)
    face, _ = check_against_reference("box", v, f, poses, 64, 64, 80.0)
    assert (face >= 0).mean() > 0.5
    # one triangle with a vertex behind the camera that covers the image: the homogeneous rule needs no clip
    v = np.array([[-60.0, -40.0, -12.0], [60.0, -40.0, -12.0], [0.0, 40.0, 8.0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    face, _ = check_against_reference("straddling triangle", v, f, np.eye(4, dtype=np.float32)[None], 64, 64, 60.0)
    assert (face == 0).all()


def test_depth_lies_on_the_ray_gen_rays_gives():
    """o + depth * dir of util.gen_rays' own rays lies on the returned face's plane: the pixel convention
    is gen_rays', whatever the test helpers assume."""
    k = R.case("A")
    poses = dev(k["poses"])
    face, depth = ops.mesh_raster(dev(k["v"]), dev(k["f"]), poses, 32, 32, k["focal"], k["c"])
    rays = util.gen_rays(poses, 32, 32, k["focal"], 0.1, 4.0, c=torch.tensor([k["c"], k["c"]]))
    pts = (rays[..., :3].double() + depth.double()[..., None] * rays[..., 3:6].double()).cpu().numpy()
    face, m = face.cpu().numpy(), k["sure"] & (k["face64"] >= 0)
    tri = k["v"].astype(np.float64)[k["f"][face[m]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    dist = np.abs(((pts[m] - tri[:, 0]) * n).sum(1))
    print("max distance from the face's plane %.3e" % dist.max())
    assert (face[m] >= 0).all() and dist.max() <= DEPTH_RTOL * k["depth64"][m].max()


def test_bit_identity():
    k = R.case("A")
    v, f, poses, s = k["v"], k["f"], k["poses"][:3], k["size"]
    bits = lambda fd: (fd[0], fd[1].view(np.int32))   # noqa: E731
    base = bits(raster(v, f, poses, s, s, k["focal"], k["c"]))
    again = bits(raster(v, f, poses, s, s, k["focal"], k["c"]))
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1])
    for n in range(3):                                   # a view alone and in the batch
        one = bits(raster(v, f, poses[n:n + 1], s, s, k["focal"], k["c"]))
        assert np.array_equal(one[0][0], base[0][n]) and np.array_equal(one[1][0], base[1][n])
    # 100 faces behind every camera: far above the upper-hemisphere cameras, which look down at the origin
    rng = np.random.default_rng(5)
    extra_v = (rng.uniform(-0.5, 0.5, (300, 3)) + [0.0, 0.0, 40.0]).astype(np.float32)
    extra_f = (np.arange(300, dtype=np.int32).reshape(100, 3) + len(v))
    more = bits(raster(np.concatenate([v, extra_v]), np.concatenate([f, extra_f]), poses, s, s, k["focal"], k["c"]))
    assert np.array_equal(more[0], base[0]) and np.array_equal(more[1], base[1])
    perm = rng.permutation(len(f))
    shuf = bits(raster(v, f[perm], poses, s, s, k["focal"], k["c"]))
    assert np.array_equal(shuf[1], base[1]) and np.array_equal(shuf[0] >= 0, base[0] >= 0)


def test_bad_faces_and_views_contribute_nothing():
    k = R.case("A")
    v, f, poses, s = k["v"], k["f"], k["poses"], k["size"]
    base = raster(v, f, poses, s, s, k["focal"], k["c"])
    v_bad = np.concatenate([v, [[np.nan, 0.0, 0.0]]]).astype(np.float32)
    nan_i, V = len(v), len(v) + 1
    bad = np.array([[0, 1, V], [0, 1, nan_i], [2, 2, 5], [-1, 0, 1], [3, 4, 3]], np.int32)
    for where in (0, len(f) // 2, len(f)):
        f_bad = np.concatenate([f[:where], bad, f[where:]])
        got = raster(v_bad, f_bad, poses, s, s, k["focal"], k["c"])
        assert np.array_equal(got[1].view(np.int32), base[1].view(np.int32))
        shifted = np.where(base[0] >= where, base[0] + len(bad), base[0])
        assert np.array_equal(got[0], shifted)
    # a camera looking away, and a non-finite pose: all -1 / 0
    away = poses.copy()
    away[:, :3, 2] *= -1
    away[:, :3, 0] *= -1
    broken = poses.copy()
    broken[1, 0, 3] = np.inf
    for p, rows in ((away, range(len(poses))), (broken, [1])):
        face, depth = raster(v, f, p, s, s, k["focal"], k["c"])
        assert (face[list(rows)] == -1).all() and (depth[list(rows)] == 0).all()
    face, depth = raster(v, f, broken, s, s, k["focal"], k["c"])
    assert np.array_equal(face[0], base[0][0]) and np.array_equal(face[2:], base[0][2:])
    # (NV, 3, 4) poses are the same cameras
    got = raster(v, f, poses[:, :3], s, s, k["focal"], k["c"])
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.int32), base[1].view(np.int32))


def test_arguments_are_checked_as_in_the_other_operations():
    k = R.case("A")
    v, f, p = dev(k["v"]), dev(k["f"]), dev(k["poses"])
    with pytest.raises(ValueError, match="HIP device"):
        ops.mesh_raster(v.cpu(), f, p, 8, 8, 8.0)
    with pytest.raises(ValueError, match="HIP device"):
        ops.mesh_raster(v, f, p.cpu(), 8, 8, 8.0)
    with pytest.raises(ValueError, match="float32"):
        ops.mesh_raster(v.double(), f, p, 8, 8, 8.0)
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_raster(v, f.long(), p, 8, 8, 8.0)
    with pytest.raises(ValueError, match="float32"):
        ops.mesh_raster(v, f, p.double(), 8, 8, 8.0)
    with pytest.raises(ValueError, match="empty mesh"):
        ops.mesh_raster(v, f[:0], p, 8, 8, 8.0)
    with pytest.raises(ValueError, match="at least one view"):
        ops.mesh_raster(v, f, p[:0], 8, 8, 8.0)
    with pytest.raises(ValueError, match=r"\(NV, 4, 4\)"):
        ops.mesh_raster(v, f, p[:, :2], 8, 8, 8.0)
    with pytest.raises(_lib.PnrError, match="not supported"):
        ops.mesh_raster(v, f, p, 8193, 8, 8.0)
    face, depth = ops.mesh_raster(v, f, p, 8, 8, 8.0)
    with pytest.raises(ValueError, match="lights"):
        ops.mesh_shade(v, f, p, 8, 8, 8.0, face, depth, lights=[(0, 0, 1)] * 9, weights=[0.1] * 9)
    with pytest.raises(ValueError, match="face must be"):
        ops.mesh_shade(v, f, p, 8, 8, 8.0, face[:, :4], depth)


LIGHTS = [(1.3, 1.3, 1.3), (-1.3, -1.3, 1.3), (0.0, -1.3, 1.3)]
WEIGHTS = [0.6, 0.2, 0.12]


def test_shading():
    k = R.case("B")
    v, f, poses, s = k["v"], k["f"], k["poses"], k["size"]
    kw = dict(lights=LIGHTS, weights=WEIGHTS, albedo=(0.9, 0.7, 0.5), ambient=0.15, background=(1.0, 0.5, 0.25))
    out = dict(zip(("face", "depth"), ops.mesh_raster(dev(v), dev(f), dev(poses), s, s, k["focal"], k["c"])))
    rgb, normal = ops.mesh_shade(dev(v), dev(f), dev(poses), s, s, k["focal"], out["face"], out["depth"], c=k["c"],
                                 want_normal=True, **kw)
    face, depth = out["face"].cpu().numpy(), out["depth"].cpu().numpy()
    rgb, normal = rgb.cpu().numpy(), normal.cpu().numpy()
    assert rgb.shape == normal.shape == (len(poses), s, s, 3) and rgb.dtype == np.float32
    # the fp64 formula on the device's own face and depth
    want_rgb, want_n = evaluate_free_shade(v, f, poses, s, k["focal"], k["c"], face, depth, np.float64, **kw)
    emul_rgb, emul_n = evaluate_free_shade(v, f, poses, s, k["focal"], k["c"], face, depth, np.float32, **kw)
    m = face >= 0
    e_rgb, e_n = np.abs(emul_rgb - want_rgb)[m].max(), np.abs(emul_n - want_n)[m].max()
    d_rgb, d_n = np.abs(rgb - want_rgb)[m].max(), np.abs(normal - want_n)[m].max()
    print("shading: emulation %.3e / %.3e, device %.3e / %.3e (rgb / normal; bounds %.1e / %.1e)"
          % (e_rgb, e_n, d_rgb, d_n, SHADE_ATOL, NORMAL_ATOL))
    assert d_rgb <= SHADE_ATOL and d_n <= NORMAL_ATOL
    bg = np.asarray(kw["background"], np.float32)
    assert (rgb[~m] == bg).all() and (normal[~m] == 0).all() and (~m).any()
    # white background: no covered pixel rounds to 255 in all channels, also with everything saturated
    hot = ops.mesh_shade(dev(v), dev(f), dev(poses), s, s, k["focal"], out["face"], out["depth"], c=k["c"],
                         lights=LIGHTS, weights=[5.0, 5.0, 5.0], albedo=(1.0, 1.0, 1.0), ambient=1.0)[0]
    img = torch.round(hot * 255.0).cpu().numpy()
    assert (img[m].max(-1) <= 254).all() and (img[~m] == 255).all() and (img[m] == 254).any()
    # without the normal, and without lights
    flat, none = ops.mesh_shade(dev(v), dev(f), dev(poses), s, s, k["focal"], out["face"], out["depth"], c=k["c"],
                                albedo=(0.5, 0.5, 0.5), ambient=0.5)
    assert none is None and (flat.cpu().numpy()[m] == 0.25).all()


def evaluate_free_shade(v, f, poses, s, focal, c, face, depth, dtype, lights, weights, albedo, ambient, background):
    """The header's shading formula in `dtype`, written out here (not pnr.evaluate's)."""
    fx, fy, cx, cy = R.cam(s, s, focal, c)
    T = dtype
    jj, ii = np.meshgrid(np.arange(s, dtype=T), np.arange(s, dtype=T), indexing="ij")
    u = np.stack([(ii - T(cx)) / T(fx), -((jj - T(cy)) / T(fy)), -np.ones_like(ii)], -1)
    u = u / np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + T(1))[..., None]
    rgb = np.zeros(face.shape + (3,), T)
    nrm = np.zeros(face.shape + (3,), T)
    rgb[:] = np.asarray(background, T)
    for n, pose in enumerate(np.asarray(poses, np.float32).astype(T)):
        m = face[n] >= 0
        tri = np.asarray(v, np.float32).astype(T)[f[face[n][m]]]
        d = (u[m][:, None, :] * pose[None, :3, :3]).sum(-1).astype(T)
        pt = pose[:3, 3] + depth[n][m].astype(T)[:, None] * d
        g = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(T)
        g = g / np.sqrt((g * g).sum(-1, keepdims=True))
        g = np.where(((g * d).sum(-1) > 0)[:, None], -g, g)
        lum = np.full(len(g), T(ambient))
        for L, w in zip(lights, weights):
            to = np.asarray(L, T) - pt
            lum = lum + T(w) * np.maximum((g * to).sum(-1) / np.sqrt((to * to).sum(-1)), T(0))
        rgb[n][m] = np.clip(np.asarray(albedo, T) * lum[:, None], T(0), T(254.0) / T(255.0))
        nrm[n][m] = g
    assert rgb.dtype == T
    return rgb.astype(np.float64), nrm.astype(np.float64)


def test_silhouette_scores():
    v, f = mesh_ref.icosphere(2, 0.45)
    poses = R.golden_poses(4, 1.3)
    same = evaluate.silhouette_scores((v, f), (v, f), poses, 32, 32, 32.8125, backend="hip")
    assert same == {"sil_iou": 1.0, "sil_depth_l1": 0.0, "sil_views": 4.0}
    small = (0.8 * v).astype(np.float32)
    got = evaluate.silhouette_scores((small, f), (v, f), poses, 32, 32, 32.8125, backend="hip")
    fa, da = R.cast64(small, f, poses, 32, 32, 32.8125)
    fb, db = R.cast64(v, f, poses, 32, 32, 32.8125)
    a, b = fa >= 0, fb >= 0
    iou = np.mean([(a[n] & b[n]).sum() / (a[n] | b[n]).sum() for n in range(4)])
    l1 = np.abs(da - db)[a & b].mean()
    print("sil_iou %.6f (reference %.6f), sil_depth_l1 %.6f (reference %.6f)" % (got["sil_iou"], iou, got["sil_depth_l1"], l1))
    # the two silhouettes may differ from the reference's on the unsure pixels only
    unsure = ~(R.sure(small, f, poses, 32, 32, 32.8125) & R.sure(v, f, poses, 32, 32, 32.8125))
    assert abs(got["sil_iou"] - iou) <= unsure.reshape(4, -1).sum(1).max() / (a | b).reshape(4, -1).sum(1).min()
    assert abs(got["sil_depth_l1"] - l1) <= 0.01 * l1 and got["sil_views"] == 4.0
    assert 0.55 < got["sil_iou"] < 0.75          # (0.8)^2 of the disc, roughly
    empty = evaluate.silhouette_scores((v[:0], f[:0]), (v, f), poses, 32, 32, 32.8125, backend="hip")
    assert empty["sil_iou"] == 0.0 and empty["sil_depth_l1"] == float("inf")


def test_render_meshes_script_writes_a_dataset_the_loader_reads(tmp_path):
    meshes, out = tmp_path / "meshes", tmp_path / "pollen"
    meshes.mkdir()
    objs = {"ball": mesh_ref.icosphere(2, 1.0), "box": R.box_mesh(2.0)}
    for name, (v, f) in objs.items():
        mesh.write_stl(str(meshes / (name + ".stl")), v, f)
    cmd = [sys.executable, os.path.join(REPO, "scripts", "render_meshes.py"), "-M", str(meshes), "-D", str(out),
           "--views", "20", "--size", "32", "--focal", "32.8125", "--object_radius", "0.5", "--ssaa", "1",
           "--backend", "hip", "--write_depth"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    gl, _ = evaluate.sphere_poses(20, 1.3)
    split = {"train": [], "val": [], "test": []}
    for i in range(20):
        split["test" if (i + 1) % 10 == 0 else "val" if (i + 1) % 10 == 1 else "train"].append(i)
    assert [len(split[k]) for k in ("train", "val", "test")] == [16, 2, 2]
    for stage, views in split.items():
        dset = SRNDataset(str(out), stage=stage, image_size=(32, 32))
        assert len(dset) == 2
        for item in dset:
            name = os.path.basename(item["path"])
            assert item["images"].shape == (len(views), 3, 32, 32) and float(item["focal"]) == np.float32(32.8125)
            assert np.array_equal(item["poses"].numpy(), gl[views].astype(np.float32))
            v, f = mesh.read_stl_indexed(str(meshes / (name + ".stl")))
            face, depth = raster(mesh.normalize_bounds(v, 0.5), f, item["poses"].numpy(), 32, 32, 32.8125)
            masks = item["masks"][:, 0].numpy() > 0
            assert np.array_equal(masks, face >= 0) and 0.1 < masks.mean() < 0.9
            saved = np.stack([np.load(os.path.join(item["path"], "depth", "%06d.npy" % n)) for n in range(len(views))])
            assert np.array_equal(saved.view(np.int32), depth.view(np.int32))
