"""Device isosurface extraction (csrc/mcubes.hip, pnr.ops.marching_cubes) against the numpy
restatement tests/mc_ref.py: verts and faces compared with np.array_equal (the semantics of
include/pnr_abi.h make the outputs bit-identical: same predicate, same three roundings per vertex,
same ownership, same order).  Then the callers: scripts/eval.py --mesh_backend hip end to end,
export_mesh in process, and the util.recon shim.

Shapes: a single cell for all 256 cases; 20 x 17 x 33 (non-cubic, no multiple of the 1024-point
run a workgroup takes or of the 64-lane wave); 71 x 70 x 69 (335 workgroups: runs that start in
the middle of a z-row and of a plane, and more than one 256-entry chunk of the scan kernel); grids
with a dimension of 1; levels outside the range; NaN planes; a surface cut by the boundary.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mc_ref
from srn_synth import write_srn_dir

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _hip(grid, level, **kw):
    from pnr import ops

    v, f = ops.marching_cubes(torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float32)).to(DEV), level, **kw)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    assert v.dim() == 2 and v.shape[1] == 3 and f.dim() == 2 and f.shape[1] == 3
    return v, f


def _check(grid, level, nonempty=True):
    v, f = _hip(grid, level)
    rv, rf = mc_ref.marching_cubes(grid, level)
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert np.array_equal(v.cpu().numpy(), rv)      # bit for bit (no NaN can appear in a vertex)
    assert np.array_equal(f.cpu().numpy(), rf)
    if nonempty:
        assert len(rv) > 0 and len(rf) > 0
    return rv, rf


def _wavy(shape, seed):
    """A smooth field with many sign changes and no symmetry, plus noise (generic t on every edge)."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    f = np.sin(0.61 * x + 0.3) * np.cos(0.47 * y - 0.2) + np.sin(0.38 * z + 0.11 * x) + 0.15 * rng.standard_normal(shape)
    return f.astype(np.float32)


def test_single_cell_every_case():
    rng = np.random.default_rng(5)
    for case in range(256):
        g = np.empty((2, 2, 2), np.float32)
        for k in range(8):
            dx, dy, dz = mc_ref.corner_xyz(k)
            mag = np.float32(0.1 + rng.random())
            g[dx, dy, dz] = mag if case >> k & 1 else -mag
        rv, rf = _check(g, 0.0, nonempty=False)
        assert len(rf) == (mc_ref.case_table()[case] >= 0).sum() // 3


def test_non_cubic_grid():
    g = _wavy((20, 17, 33), 0)
    _check(g, 0.0)
    _check(g, 0.37)
    # each axis order once more: a transposed grid is another grid, not the same mesh
    _check(np.ascontiguousarray(g.transpose(2, 0, 1)), -0.2)


def test_many_workgroups_and_scan_chunks():
    shape = (71, 70, 69)
    assert shape[0] * shape[1] * shape[2] > 256 * 1024     # more than one chunk of the scan kernel
    g = _wavy(shape, 1)
    rv, rf = _check(g, 0.1)
    assert len(rv) > 100000


def test_empty_results():
    g = _wavy((9, 10, 11), 2)
    for shape in ((1, 10, 11), (9, 1, 11), (9, 10, 1), (1, 1, 1)):
        v, f = _hip(g[:shape[0], :shape[1], :shape[2]], 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    for level in (float(g.max()) + 1.0, float(g.max()), float(g.min()) - 1.0):
        v, f = _hip(g, level)       # a level equal to the maximum: nothing is > level
        assert v.shape == (0, 3) and f.shape == (0, 3)
        _check(g, level, nonempty=False)


def test_nan_planes_are_outside():
    g = _wavy((20, 17, 33), 3) + np.float32(0.4)
    g[7, :, :] = np.nan
    g[:, 11, :] = np.nan
    g[:, :, 20] = np.nan
    g[3, 4, 5] = np.inf
    g[12, 3, 9] = -np.inf
    rv, rf = _check(g, 0.0)
    assert np.isfinite(rv).all()


def test_surface_cut_by_the_boundary_stays_open():
    g = mc_ref.sphere_grid((18, 16, 21), (2.3, 8.2, 17.9), 6.4)
    rv, rf = _check(g, 0.0)
    assert not mc_ref.is_closed_oriented(rf)


CLOSED = {
    "sphere": (lambda: mc_ref.sphere_grid((24, 25, 26), (11.3, 12.7, 12.1), 8.3), 2),
    "torus": (lambda: mc_ref.torus_grid((26, 27, 12), (12.4, 13.1, 5.6), 7.2, 3.1), 0),
    "two_spheres": (lambda: mc_ref.two_spheres_grid((30, 16, 15), (7.2, 7.9, 7.4), 5.3, (21.6, 8.1, 7.3), 5.8), 4),
}


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_fixtures(name):
    make, chi = CLOSED[name]
    g = make()
    _check(g, 0.0)
    v, f = _hip(g, 0.0)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert mc_ref.is_closed_oriented(f)       # every undirected edge in two faces, opposite directions
    assert mc_ref.euler(v, f) == chi
    assert mc_ref.signed_volume(v, f) > 0


def test_edge_map_index_past_2_31():
    """1024 x 1024 x 700: 3 n = 2.2e9 edge-map entries, so the entries of the last grid points lie
    past 2^31 (and past 2^33 in bytes), where the blob is, and the scan kernel walks 716,800
    workgroup counts in 2,800 chunks.  mc_ref runs on the blob's block alone."""
    from pnr import ops

    shape, sub = (1024, 1024, 700), (12, 11, 13)
    assert 3 * shape[0] * shape[1] * shape[2] > 2 ** 31
    blob = mc_ref.sphere_grid(sub, (6.2, 5.4, 6.7), 3.6)
    assert blob[0].max() < 0 and blob[:, 0].max() < 0 and blob[:, :, 0].max() < 0   # no crossing into the fill
    off = tuple(s - b for s, b in zip(shape, sub))
    g = torch.full(shape, -1.0, device=DEV)
    g[off[0]:, off[1]:, off[2]:] = torch.from_numpy(blob).to(DEV)
    v, f = ops.marching_cubes(g, 0.0)
    rv, rf = mc_ref.marching_cubes(blob, 0.0, index_offset=off)
    assert len(rf) > 100
    assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(f.cpu().numpy(), rf)
    v, f = ops.marching_cubes(g.flip(0, 1, 2).contiguous(), 0.0)      # the same blob in the first cells
    rv, rf = mc_ref.marching_cubes(blob[::-1, ::-1, ::-1], 0.0)
    assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(f.cpu().numpy(), rf)


def test_back_to_back_calls_are_identical_and_transform():
    g = torch.from_numpy(_wavy((40, 37, 45), 4)).to(DEV)
    from pnr import ops

    v0, f0 = ops.marching_cubes(g, 0.05)
    v1, f1 = ops.marching_cubes(g, 0.05)
    assert v0.shape[0] > 0 and torch.equal(v0, v1) and torch.equal(f0, f1)
    v2, f2 = ops.marching_cubes(g, 0.05, spacing=(0.5, 2.0, 0.25), origin=(-1.0, 3.0, 0.5))
    want = v0 * torch.tensor([0.5, 2.0, 0.25], device=DEV) + torch.tensor([-1.0, 3.0, 0.5], device=DEV)
    assert torch.equal(v2, want) and torch.equal(f2, f0)
    with pytest.raises(ValueError):
        ops.marching_cubes(g.cpu(), 0.05)


def test_short_capacities_return_an_error_and_leave_the_tail_untouched():
    from pnr import _lib

    lib = _lib.load()
    grid = _wavy((20, 17, 33), 0)
    rv, rf = mc_ref.marching_cubes(grid, 0.0)
    g = torch.from_numpy(grid).to(DEV)
    nbytes = lib.pnr_mc_workspace_bytes(20, 17, 33)
    assert nbytes >= 12 * 20 * 17 * 33
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    counts = torch.empty(2, device=DEV, dtype=torch.int64)
    st = _lib.stream_of(DEV)
    assert lib.pnr_mc_count(_lib.ptr(g), 20, 17, 33, 0.0, _lib.ptr(ws), nbytes, _lib.ptr(counts), st) == 0
    n_v, n_t = counts.cpu().tolist()
    assert (n_v, n_t) == (len(rv), len(rf))
    # a workspace one byte short is refused before any launch
    assert lib.pnr_mc_count(_lib.ptr(g), 20, 17, 33, 0.0, _lib.ptr(ws), nbytes - 1, _lib.ptr(counts), st) == -4
    for cap_v, cap_t in ((n_v // 2, n_t), (n_v, n_t // 3), (0, 0), (n_v - 1, n_t - 1)):
        verts = torch.full((n_v, 3), -77.0, device=DEV)
        faces = torch.full((n_t, 3), -77, device=DEV, dtype=torch.int32)
        rc = lib.pnr_mc_emit(_lib.ptr(g), 20, 17, 33, 0.0, _lib.ptr(ws), nbytes, _lib.ptr(verts), cap_v,
                             _lib.ptr(faces), cap_t, st)
        assert rc == -1 and b"capacities" in lib.pnr_last_error()
        torch.cuda.synchronize()
        assert bool((verts[cap_v:] == -77.0).all()) and bool((faces[cap_t:] == -77).all())
        assert np.array_equal(verts[:cap_v].cpu().numpy(), rv[:cap_v])
        if cap_v == n_v:
            assert np.array_equal(faces[:cap_t].cpu().numpy(), rf[:cap_t])
    verts = torch.full((n_v + 5, 3), -77.0, device=DEV)
    faces = torch.full((n_t + 5, 3), -77, device=DEV, dtype=torch.int32)
    assert lib.pnr_mc_emit(_lib.ptr(g), 20, 17, 33, 0.0, _lib.ptr(ws), nbytes, _lib.ptr(verts), n_v + 5,
                           _lib.ptr(faces), n_t + 5, st) == 0
    assert np.array_equal(verts[:n_v].cpu().numpy(), rv) and np.array_equal(faces[:n_t].cpu().numpy(), rf)
    assert bool((verts[n_v:] == -77.0).all()) and bool((faces[n_t:] == -77).all())


# ---- the callers ---------------------------------------------------------------------------------
# the conf of tests/test_data_eval.py's script tests (a copy: that file stays as it is)
CLI_CONF = """
model {
    use_encoder = True
    use_xyz = True
    use_code = True
    code { num_freqs = 6, freq_factor = 1.5, include_input = True }
    use_viewdirs = True
    use_code_viewdirs = False
    mlp_coarse { type = resnet, n_blocks = 5, d_hidden = 512, combine_layer = 3, combine_type = average }
    mlp_fine { type = resnet, n_blocks = 5, d_hidden = 512, combine_layer = 3, combine_type = average }
    encoder { backbone = resnet34, pretrained = False, num_layers = 4 }
}
renderer {
    n_coarse = 32
    n_fine = 16
    n_fine_depth = 8
    depth_std = 0.01
    white_bkgd = True
}
"""


def _golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "srn_loader.npz")))


def _synth_setup(tmp_path):
    from pnr import synth
    from pnr.conf import parse_file
    from pnr.models import make_model

    root = write_srn_dir(str(tmp_path), _golden())
    (tmp_path / "exp.conf").write_text(CLI_CONF)
    ck = tmp_path / "ck" / "synthnet"
    ck.mkdir(parents=True)
    net = make_model(parse_file(str(tmp_path / "exp.conf"))["model"])
    full = net.state_dict()
    sd = synth.pixelnerf_state(2)
    # the hash-initialised net's sigma is negative over the whole [-1, 1]^3 cube (an all-zero grid
    # after the relu); with its sigma row negated the grid has a surface to extract
    for k in ("mlp_coarse.lin_out.weight", "mlp_coarse.lin_out.bias"):
        sd[k] = sd[k].clone()
        sd[k][3] = -sd[k][3]
    full.update(sd)
    torch.save(full, str(ck / "pixel_nerf_latest"))
    net.load_state_dict(full)
    return root, net


def _eval_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("pnr_scripts_eval", os.path.join(REPO, "scripts", "eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stl_triangles(path):
    from pnr import mesh

    size = os.path.getsize(path)
    normals, tris = mesh.read_stl(path)
    assert size == 84 + 50 * len(tris)
    return normals, tris


def test_eval_script_writes_the_mesh(tmp_path):
    """scripts/eval.py --mesh_backend hip --compare on the synthetic SRN set: per object an STL of
    84 + 50 T bytes whose triangles are mc_ref's on the saved grid, and a finish.txt line.  The
    threshold is the median of the first object's positive densities, computed here with the query
    the script runs (the reference's default 0.1 says nothing about a synthetic net)."""
    from pnr.data import get_split_dataset

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
    assert (sig0 > 0).any(), "the synthetic net's density grid is all zero"
    thresh = float(np.median(sig0[sig0 > 0]))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "eval.py"), "-c", str(tmp_path / "exp.conf"),
                        "-D", root, "-n", "synthnet", "--checkpoints_path", str(tmp_path / "ck"), "--split", "test",
                        "-P", "0 1", "--mesh_res", "20", "--mesh_thresh", repr(thresh), "--mesh_backend", "hip",
                        "--compare", "-O", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ERROR" not in r.stdout, r.stdout[-3000:]
    assert r.stdout.count("mesh (hip)") == len(names)
    lines = (out / "finish.txt").read_text().strip().splitlines()
    assert [ln.split()[0] for ln in lines] == names
    for i, n in enumerate(names):
        sig = np.load(str(out / n / (n + "_sigma.npy")))
        rv, rf = mc_ref.marching_cubes(sig, thresh)
        normals, tris = _stl_triangles(str(out / n / (n + "_mesh.stl")))
        assert np.array_equal(tris, rv[rf])
        if i == 0:
            assert len(rf) > 0


def test_export_mesh_in_process(tmp_path):
    ev = _eval_module()
    grid = mc_ref.sphere_grid((24, 25, 26), (11.3, 12.7, 12.1), 8.3)
    path = str(tmp_path / "sphere.stl")
    backend, n_tri, dt = ev.export_mesh(torch.from_numpy(grid).to(DEV), 0.0, path, backend="hip")
    rv, rf = mc_ref.marching_cubes(grid, 0.0)
    normals, tris = _stl_triangles(path)
    assert backend == "hip" and n_tri == len(rf) > 0 and dt >= 0
    assert np.array_equal(tris, rv[rf])
    # facet normals: unit, along the right-hand normal, pointing away from the centre
    n64 = np.cross(tris[:, 1] - tris[:, 0].astype(np.float64), tris[:, 2] - tris[:, 0].astype(np.float64))
    area = np.linalg.norm(n64, axis=1)
    ok = area > 0
    np.testing.assert_allclose(normals[ok], (n64[ok] / area[ok, None]).astype(np.float32), atol=1e-6)
    assert (normals[~ok] == 0).all()
    out = tris.mean(1) - np.array([11.3, 12.7, 12.1])
    assert (np.einsum("ij,ij->i", normals[ok], out[ok]) > 0).all()
    # a threshold outside the range: a valid empty STL, no exception
    backend, n_tri, dt = ev.export_mesh(torch.from_numpy(grid).to(DEV), 1e30, path, backend="hip")
    assert n_tri == 0 and os.path.getsize(path) == 84 and len(_stl_triangles(path)[1]) == 0


def test_util_recon_shim(tmp_path):
    """util.recon.marching_cubes on the synthetic net: the reference's grid (gen_grid 'ij'), fake
    view directions, (c2 - c1) / reso scaling and + c1 offset (recon.py:43-78)."""
    import util.recon as recon
    from pnr.data import get_split_dataset
    from pnr.util import gen_grid

    root, net = _synth_setup(tmp_path)
    net = net.to(DEV).eval()
    data = get_split_dataset("srn", root, want_split="test", training=False)[0]
    focal = torch.as_tensor(data["focal"], dtype=torch.float32)[None].to(DEV)
    c1, c2, reso = [-1.0, -0.9, -0.8], [1.0, 0.8, 0.9], [12, 13, 14]
    with torch.no_grad():
        net.encode(data["images"][:2].to(DEV)[None], data["poses"][:2].to(DEV)[None], focal,
                   c=data["c"].to(DEV)[None])
        pts = gen_grid(*zip(c1, c2, reso), ij_indexing=True).to(DEV)
        vd = -pts / torch.norm(pts, dim=-1).unsqueeze(-1)
        sig = net(pts[None], coarse=True, viewdirs=vd[None])[0, :, 3].view(*reso).cpu().numpy()
    iso = float(np.median(sig[sig > 0]))
    with pytest.warns(UserWarning):
        vertices, triangles = recon.marching_cubes(net, c1, c2, reso, isosurface=iso, eval_batch_size=700)
    rv, rf = mc_ref.marching_cubes(sig, iso)
    assert len(rf) > 0
    assert vertices.shape == rv.shape and vertices.dtype == np.float64
    assert triangles.shape == rf.shape and np.array_equal(triangles, rf)
    want = rv.astype(np.float64) * ((np.array(c2) - np.array(c1)) / np.array(reso)) + np.array(c1)
    assert np.array_equal(vertices, want)
    recon.save_obj(vertices, triangles, str(tmp_path / "m.obj"))
    lines = (tmp_path / "m.obj").read_text().splitlines()
    assert len(lines) == len(vertices) + len(triangles)
    assert lines[0] == "v %.4f %.4f %.4f" % tuple(vertices[0])
    assert lines[-1] == "f %d %d %d" % tuple(triangles[-1] + 1)
