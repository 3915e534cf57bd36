"""Device mesh cleanup (csrc/meshclean.hip; pnr.ops.mesh_weld / mesh_components /
mesh_component_stats, pnr.evaluate.clean_mesh backend "hip") against tests/meshclean_ref.py: the
integer outputs (remaps, labels, counts, kept sets) compared for equality with the np.unique / scipy
references, the fp64 sums within the summation-order bound, every output bit-identical from run to run
and inside a concatenation, then scripts/eval.py --components largest --write_clean_mesh end to end.

Shapes: B = ops.MESH_CLEAN_BLOCK threads take one vertex or face each, so V and T in {1, B - 1, B,
B + 1, 2 B + 5} cover a partial, a full and several workgroups; 1,000 copies of one point put all the
weld's contention on one slot and 4,096 lattice points stress its probing; the 4,097-vertex strips are
the long chains of the union-find, the 2,000-face fan its contention on one root."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshclean_ref as ref
import mesh_ref
from pnr import _lib, evaluate, mesh, ops

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
B = ops.MESH_CLEAN_BLOCK
SIZES = (1, B - 1, B, B + 1, 2 * B + 5)

_MESHES = {}


def meshes():
    if not _MESHES:
        _MESHES.update(ref.shared_meshes())
    return _MESHES


def dev(v, f=None):
    tv = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV)
    return tv if f is None else (tv, torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV))


def host(t):
    return t.cpu().numpy()


def hip_remap(v):
    r = ops.mesh_weld_remap(dev(v))
    assert r.dtype == torch.int32 and r.is_cuda and tuple(r.shape) == (len(v),)
    return host(r)


def hip_components(n_verts, f):
    vl, fl, n, launches = ops.mesh_components(n_verts, dev(np.zeros((1, 3)), f)[1], return_launches=True)
    assert vl.dtype == fl.dtype == torch.int32 and tuple(vl.shape) == (n_verts,) and tuple(fl.shape) == (len(f),)
    return host(vl), host(fl), n, launches


def check_components(n_verts, f):
    vl, fl, n, launches = hip_components(n_verts, f)
    rv, rf, rn = ref.components(n_verts, f)
    assert np.array_equal(vl, rv) and np.array_equal(fl, rf) and n == rn
    return launches


# ---- weld ------------------------------------------------------------------------------------------
def test_weld_icosphere_soup():
    v, f = mesh_ref.icosphere(3)
    sv, sf = ref.soup(v, f)
    wv, wf, remap = ops.mesh_weld(*dev(sv, sf))
    assert len(sv) == 3840 and tuple(wv.shape) == (642, 3) and tuple(wf.shape) == (1280, 3) and wf.dtype == torch.int32
    rv, rf, rr = ref.weld_mesh(sv, sf)
    assert np.array_equal(host(remap), rr) and np.array_equal(host(wv), rv) and np.array_equal(host(wf), rf)
    assert np.array_equal(host(wv)[host(wf)], v[f])      # the same triangles, record for record


@pytest.mark.parametrize("n", SIZES)
def test_weld_sizes(n):
    rng = np.random.default_rng(n)
    pool = rng.integers(-4, 5, ((n + 2) // 3, 3)).astype(np.float32) * np.float32(0.37)
    v = pool[rng.integers(0, len(pool), n)]
    assert np.array_equal(hip_remap(v), ref.weld(v))
    f = rng.integers(0, n, (7, 3)).astype(np.int32)
    wv, wf, remap = ops.mesh_weld(*dev(v, f))
    rv, rf, rr = ref.weld_mesh(v, f)
    assert np.array_equal(host(wv), rv) and np.array_equal(host(wf), rf) and np.array_equal(host(remap), rr)


def test_weld_one_point_a_thousand_times():
    v = np.tile(np.array([[0.25, -3.0, 7.5]], np.float32), (1000, 1))
    assert not hip_remap(v).any()
    wv, wf, _ = ops.mesh_weld(*dev(v, np.arange(999, dtype=np.int32).reshape(-1, 3)))
    assert tuple(wv.shape) == (1, 3) and not host(wf).any() and tuple(wf.shape) == (333, 3)


def test_weld_signed_zero_nan_and_inf():
    v = np.array([[0.0, 1, 2], [-0.0, 1, 2], [np.nan, 0, 0], [np.nan, 0, 0], [0, 1, 2], [5, 5, 5], [0, -0.0, 0],
                  [0, 0, -0.0], [np.inf, 0, 0], [np.inf, 0, 0], [1, np.nan, 1], [1, np.nan, 1]], np.float32)
    want = [0, 0, 2, 3, 0, 5, 6, 6, 8, 8, 10, 11]
    assert ref.weld(v).tolist() == want and hip_remap(v).tolist() == want


def test_weld_lattice_is_the_identity():
    g = np.arange(16, dtype=np.float32)
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    assert len(v) == 4096 and np.array_equal(hip_remap(v), np.arange(4096))
    v2 = np.concatenate([v, v[::-1]])            # and every point twice, the copies in reverse order
    assert np.array_equal(hip_remap(v2), np.concatenate([np.arange(4096), np.arange(4096)[::-1]]))


def test_weld_refuses_bad_faces_and_empty_input():
    v = dev(np.eye(3, dtype=np.float32))
    for bad in (3, -1):
        with pytest.raises(ValueError, match="outside"):
            ops.mesh_weld(v, torch.tensor([[0, 1, bad]], dtype=torch.int32, device=DEV))
    wv, wf, remap = ops.mesh_weld(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert tuple(wv.shape) == (0, 3) and tuple(wf.shape) == (0, 3) and tuple(remap.shape) == (0,)


# ---- components --------------------------------------------------------------------------------------
def test_components_without_faces():
    vl, fl, n, launches = hip_components(5, np.zeros((0, 3), np.int32))
    assert vl.tolist() == [0, 1, 2, 3, 4] and fl.shape == (0,) and n == 5 and launches == 2


def test_components_one_face():
    vl, fl, n, launches = hip_components(6, np.array([[5, 2, 4]], np.int32))
    assert vl.tolist() == [0, 1, 2, 3, 2, 2] and fl.tolist() == [2] and n == 4 and launches == 3


@pytest.mark.parametrize("name", ["two_shuffled", "strip_reversed", "strip_random", "fan", "blob_grid",
                                  "three_spheres", "floater"])
def test_components_match_scipy(name):
    v, f = meshes()[name]
    launches = check_components(len(v), f)
    print("%s: V %d, T %d, %d components, %d launches" % (name, len(v), len(f), ref.components(len(v), f)[2], launches))
    if name == "two_shuffled":
        vl = ref.components(len(v), f)[0]
        assert len(np.unique(vl)) == 2 and vl.min() == 0
    if name.startswith("strip"):
        assert len(v) == 4097 and ref.components(len(v), f)[2] == 1
    if name == "blob_grid":
        assert ref.components(len(v), f)[2] == 23


@pytest.mark.parametrize("n", (B - 1, B + 1, 2 * B + 5))
def test_components_sizes(n):
    # n islands, then the same faces chained into one strip-like component through shared vertices
    v, f = ref.islands(n)
    assert check_components(len(v), f) == 3
    rng = np.random.default_rng(n)
    g = rng.integers(0, n + 2, (n, 3)).astype(np.int32)      # a random sparse graph: many small components
    check_components(n + 2, g)
    sv, sf = ref.strip(n + 2, "random", seed=n)
    assert len(sf) == n
    check_components(len(sv), sf)


@pytest.mark.parametrize("bad", ("V", -1))
def test_components_refuse_a_bad_index(bad):
    v, f = mesh_ref.icosphere(1)
    f = f.copy()
    f[37, 1] = len(v) if bad == "V" else -1
    with pytest.raises(_lib.PnrError, match="outside"):
        ops.mesh_components(len(v), dev(v, f)[1])
    # and the next call is unaffected
    check_components(len(v), mesh_ref.icosphere(1)[1])


@pytest.mark.parametrize("name", ["floater", "blob_grid"])
def test_weld_then_components_is_the_indexed_partition(name):
    v, f = meshes()[name]
    sv, sf = meshes()[name + "_soup"]
    wv, wf, _ = ops.mesh_weld(*dev(sv, sf))
    fl_soup = host(ops.mesh_components(wv, wf)[1])
    fl_indexed = host(ops.mesh_components(len(v), dev(v, f)[1])[1])
    assert ref.same_partition(fl_soup, fl_indexed)
    assert not ref.same_partition(fl_soup, np.arange(len(sf)))          # welded: no longer one per triangle
    assert ops.mesh_components(len(sv), dev(sv, sf)[1])[2] == len(sf)         # the raw soup is


# ---- statistics ----------------------------------------------------------------------------------------
def hip_stats(v, f):
    tv, tf = dev(v, f)
    vl, fl, _ = ops.mesh_components(tv, tf)
    st = ops.mesh_component_stats(tv, tf, vl, fl)
    assert tuple(st) == ops.COMPONENT_STAT_KEYS
    assert st["n_verts"].dtype == st["n_faces"].dtype == torch.int64
    assert st["area"].dtype == st["signed_volume"].dtype == torch.float64
    return {k: host(t) for k, t in st.items()}


@pytest.mark.parametrize("name", ["three_spheres", "blob_grid", "two_shuffled", "fan", "no_faces", "floater_soup"])
def test_component_stats(name):
    v, f = meshes()[name]
    st = hip_stats(v, f)
    rv, rf, _ = ref.components(len(v), f)
    rs = ref.stats(v, f, rv, rf)
    for key in ("labels", "n_verts", "n_faces"):
        assert np.array_equal(st[key], rs[key]), key
    assert np.array_equal(st["labels"][st["vert_id"]], rv) and np.array_equal(st["labels"][st["face_id"]], rf)
    worst = 0.0
    for key in ("area", "signed_volume"):
        bound = rs["n_faces"] * 2.0 ** -52 * rs["abs_" + key]
        err = np.abs(st[key] - rs[key])
        worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
        assert (err <= bound).all(), (key, err.max())
    print("%s: %d components, max |hip - numpy| / bound = %.3g" % (name, len(rs["labels"]), worst))
    if name == "three_spheres":
        assert st["n_faces"].tolist() == [1280, 320, 80] and (st["signed_volume"] > 0).all()
        assert st["area"][0] < st["area"][1] < st["area"][2]


def test_stats_of_a_component_larger_than_one_pass():
    """5,120 faces in one component: more than the 1,024 faces one pass of the sum workgroup takes."""
    v, f = mesh_ref.icosphere(4, 2.0)
    st = hip_stats(v, f)
    ta, tv = ref.face_terms(v, f)
    assert st["n_faces"].tolist() == [5120] and st["n_verts"].tolist() == [2562]
    assert abs(st["area"][0] - ta.sum()) <= 5120 * 2.0 ** -52 * ta.sum()
    assert abs(st["signed_volume"][0] - tv.sum() / 6) <= 5120 * 2.0 ** -52 * np.abs(tv).sum() / 6
    assert abs(st["signed_volume"][0] - 4 / 3 * np.pi * 8) <= 0.02 * 4 / 3 * np.pi * 8


# ---- determinism ---------------------------------------------------------------------------------------
def everything(v, f):
    """Every device output of the chain on the soup of (v, f), as host arrays."""
    sv, sf = ref.soup(v, f)
    wv, wf, remap = ops.mesh_weld(*dev(sv, sf))
    vl, fl, n = ops.mesh_components(wv, wf)
    st = ops.mesh_component_stats(wv, wf, vl, fl)
    out = {"remap": remap, "wv": wv, "wf": wf, "vl": vl, "fl": fl}
    out.update(st)
    return {k: host(t) for k, t in out.items()}, n


def test_outputs_are_bit_identical_across_runs_and_inside_a_concatenation():
    a = meshes()["blob_grid"]
    b = ref.permuted(*meshes()["three_spheres"], seed=4)[:2]
    b = (b[0] + np.array([100, 0, 0], np.float32), b[1])          # disjoint from a's coordinates
    one, n_one = everything(*a)
    two, n_two = everything(*a)
    assert n_one == n_two == 23
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k             # bitwise, floats included
    # a after b: every index of a shifted by b's sizes, every value the same bits
    both, n_both = everything(*ref.concat(b, a))
    alone_b, n_b = everything(*b)
    assert n_both == n_one + n_b
    sv_off, wv_off, t_off, c_off = 3 * len(b[1]), len(alone_b["wv"]), len(b[1]), n_b
    assert np.array_equal(both["remap"][sv_off:] - sv_off, one["remap"])
    assert both["wv"][wv_off:].tobytes() == one["wv"].tobytes()
    assert np.array_equal(both["wf"][t_off:] - wv_off, one["wf"])
    assert np.array_equal(both["vl"][wv_off:] - wv_off, one["vl"]) and np.array_equal(both["fl"][t_off:] - wv_off, one["fl"])
    assert np.array_equal(both["labels"][c_off:] - wv_off, one["labels"])
    for k in ("n_verts", "n_faces", "area", "signed_volume"):
        assert both[k][c_off:].tobytes() == one[k].tobytes(), k
        assert both[k][:c_off].tobytes() == alone_b[k].tobytes(), k


# ---- clean_mesh: hip against numpy ---------------------------------------------------------------------
def both_backends(v, f, **kw):
    hv, hf, hinfo = evaluate.clean_mesh(*dev(v, f), backend="hip", **kw)
    assert hv.is_cuda and hf.is_cuda and hv.dtype == torch.float32 and hf.dtype == torch.int32
    nv, nf, ninfo = evaluate.clean_mesh(v, f, backend="numpy", **kw)
    assert host(hv).tobytes() == nv.tobytes() and np.array_equal(host(hf), nf) and hinfo == ninfo
    return hv, hf, hinfo


def test_clean_mesh_parity_on_the_floater_scenario():
    clean, dirty = ref.floater_scene()
    hv, hf, info = both_backends(*dirty, keep="largest")
    assert info == {"n_components": 2, "n_components_kept": 1, "faces_kept": 1280}
    assert np.array_equal(host(hv), clean[0]) and np.array_equal(host(hf), clean[1])
    both_backends(*ref.soup(*dirty), keep="largest")
    both_backends(*ref.soup(*dirty), weld=False, keep="largest")
    # a host mesh goes to the device; the metrics of the cleaned mesh are those of the clean mesh, bit for bit
    cv, cf, _ = evaluate.clean_mesh(*dirty, backend="hip")
    gt = dev(*clean)
    kw = dict(n_samples=4000, tau=0.01, backend="hip")
    assert evaluate.mesh_metrics((cv, cf), gt, **kw) == evaluate.mesh_metrics(gt, gt, **kw)
    assert evaluate.mesh_metrics(dev(*dirty), gt, **kw) != evaluate.mesh_metrics(gt, gt, **kw)
    kw = dict(n_points=4000, backend="hip")
    assert evaluate.volume_iou((cv, cf), gt, **kw) == evaluate.volume_iou(gt, gt, **kw)


@pytest.mark.parametrize("kw", [dict(keep="largest"), dict(keep="largest", by="area"), dict(keep="all"),
                                dict(keep="all", min_frac=0.05), dict(keep="all", min_frac=0.5, by="area")],
                         ids=lambda kw: "-".join("%s" % v for v in kw.values()))
def test_clean_mesh_parity_on_the_grid_mesh(kw):
    v, f = meshes()["blob_grid"]
    hv, hf, info = both_backends(v, f, **kw)
    assert info["n_components"] == 23
    if kw == dict(keep="all", min_frac=0.05):
        assert info["n_components_kept"] == 3          # the spikes have 8 faces each
    both_backends(*meshes()["blob_grid_soup"], **kw)


def test_clean_mesh_parity_on_three_spheres_and_empty_meshes():
    v, f = meshes()["three_spheres"]
    assert both_backends(v, f, keep="all", min_frac=0.25)[2]["faces_kept"] == 1600
    assert both_backends(v, f, keep="all", min_frac=0.1, by="area")[2]["faces_kept"] == 400
    assert both_backends(v, f, keep="largest", by="area")[2]["faces_kept"] == 80
    e = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    for m in (e, (np.ones((4, 3), np.float32), e[1])):
        hv, hf, info = both_backends(*m)
        assert tuple(hv.shape) == (0, 3) and tuple(hf.shape) == (0, 3)
        assert info == {"n_components": 0, "n_components_kept": 0, "faces_kept": 0}


# ---- scripts/eval_mesh.py, scripts/eval.py ---------------------------------------------------------------
def test_eval_mesh_script_cleans_on_the_device(tmp_path):
    """scripts/eval_mesh.py --components largest --metrics_backend hip: the STL soup of "b" (the sphere
    of "a" plus a far floater) is welded and filtered on the device, so "b" scores as "a" to the bit and
    the counts are those of the numpy backend (tests/test_mesh_clean.py)."""
    res = 33
    out, gt = mesh_ref.write_eval_tree(str(tmp_path), res, {"a": (0.5, 1.0), "b": (0.5, 1.0)})
    fv, ff = mesh_ref.icosphere(0, 0.01)
    dv, df = ref.concat(mesh_ref.icosphere(3, 0.5), (fv + np.array([0.95, 0, 0], np.float32), ff))
    mesh.write_stl(os.path.join(out, "b", "b_mesh.stl"), mesh_ref.to_index_units(dv, res), df)
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "eval_mesh.py"), "-O", out, "-G", gt, "--mesh_res",
                        str(res), "--n_samples", "1500", "--tau", "0.05", "--components", "largest", "--metrics_backend",
                        "hip"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "hip backend" in r.stdout
    rows = {}
    for k in ("a", "b"):
        with open(os.path.join(out, k, "mesh_metrics.txt")) as fh:
            rows[k] = {ln.split()[0]: float(ln.split()[1]) for ln in fh}
        assert list(rows[k]) == list(evaluate.MESH_METRIC_NAMES) + list(evaluate.CLEAN_INFO_NAMES)
    assert [rows["a"][k] for k in evaluate.CLEAN_INFO_NAMES] == [1.0, 1.0, 1280.0]
    assert [rows["b"][k] for k in evaluate.CLEAN_INFO_NAMES] == [2.0, 1.0, 1280.0]
    assert all(rows["b"][k] == rows["a"][k] for k in evaluate.MESH_METRIC_NAMES)



def test_eval_script_cleans_the_device_mesh(tmp_path):
    """scripts/eval.py --gt_mesh_dir --components largest --write_clean_mesh on the synthetic SRN set
    (driven as tests/test_gpu_mcubes.py drives it): both STLs per object, the clean one exactly the
    faces of the raw STL's largest component (welded soup, scipy labels, most faces, lowest label on a
    tie) in their order, and the component counts at the end of mesh_metrics.txt."""
    from test_gpu_mcubes import _eval_module, _stl_triangles, _synth_setup

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
    thresh = float(np.median(sig0[sig0 > 0]))
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    mesh.write_stl(str(gt_dir / (names[0] + ".stl")), *mesh_ref.icosphere(2))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "eval.py"), "-c", str(tmp_path / "exp.conf"),
                        "-D", root, "-n", "synthnet", "--checkpoints_path", str(tmp_path / "ck"), "--split", "test",
                        "-P", "0 1", "--mesh_res", "20", "--mesh_thresh", repr(thresh), "--mesh_backend", "hip",
                        "--gt_mesh_dir", str(gt_dir), "--n_samples", "2000", "--components", "largest",
                        "--write_clean_mesh", "-O", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ERROR" not in r.stdout, r.stdout[-3000:]
    for i, n in enumerate(names):
        _, raw = _stl_triangles(str(out / n / (n + "_mesh.stl")))
        _, clean = _stl_triangles(str(out / n / (n + "_mesh_clean.stl")))
        sv = raw.reshape(-1, 3)
        wv, wf, _ = ref.weld_mesh(sv, np.arange(len(sv)).reshape(-1, 3))
        fl = ref.components(len(wv), wf)[1]
        labels, counts = np.unique(fl, return_counts=True)
        keep = fl == labels[np.argmax(counts)] if len(fl) else np.zeros(0, bool)
        assert np.array_equal(clean, raw[keep])
        print("%s: %d triangles in %d components, %d kept" % (n, len(raw), len(labels), int(keep.sum())))
        if i == 0:
            assert len(raw) > 0
            rows = [ln.split() for ln in (out / n / "mesh_metrics.txt").read_text().splitlines()]
            assert [row[0] for row in rows] == list(evaluate.MESH_METRIC_NAMES) + list(evaluate.CLEAN_INFO_NAMES)
            assert [float(row[1]) for row in rows[-3:]] == [float(len(labels)), 1.0, float(keep.sum())]
        else:
            assert not (out / n / "mesh_metrics.txt").exists()
    # the flag needs something to clean with
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "eval.py"), "-c", str(tmp_path / "exp.conf"),
                        "-D", root, "--write_clean_mesh"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "write_clean_mesh" in r.stderr
