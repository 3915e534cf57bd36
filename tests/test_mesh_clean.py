"""Host side of the mesh cleanup (no GPU): the new ABI entries and their refusals through the ctypes
binding, pnr.evaluate's numpy backend (weld_np / components_np / component_stats_np / clean_mesh)
against tests/meshclean_ref.py, the floater scenario end to end through mesh_metrics and volume_iou,
and scripts/eval_mesh.py --components / --min_component_frac.  The device kernels are
tests/test_gpu_mesh_clean.py's."""
import os
import re
import sys

import numpy as np
import pytest

import meshclean_ref as ref
import mesh_ref
from mesh_ref import _lines, _run
from pnr import _lib, evaluate, mesh, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NEW_SYMBOLS = ("pnr_mesh_weld_workspace_bytes", "pnr_mesh_weld", "pnr_mesh_components_workspace_bytes",
               "pnr_mesh_components", "pnr_mesh_component_sums")

_MESHES = {}


def meshes():
    if not _MESHES:
        _MESHES.update(ref.shared_meshes())
    return _MESHES


def test_library_exports_the_new_symbols_at_abi_8():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 8 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    text = open(os.path.join(REPO, "include", "pnr_abi.h")).read()
    assert "Mesh cleanup" in text
    defs = {k: int(v) for k, v in re.findall(r"#define (PNR_[A-Z_]+) (\d+)", text)}
    assert ops.MESH_CLEAN_BLOCK == defs["PNR_MESH_CLEAN_BLOCK"]


def test_abi_entries_refuse_bad_sizes_and_null_arguments():
    lib = _lib.load()
    err = lib.pnr_last_error
    wb, cb = lib.pnr_mesh_weld_workspace_bytes, lib.pnr_mesh_components_workspace_bytes
    assert wb(0) == 0 and b"pnr_mesh_weld" in err()
    assert wb(2 ** 29 + 1) == 0 and wb(-3) == 0
    # the table: a power of two >= 2 V slots of 4 bytes
    for n in (1, 100, 128, 129, 5000):
        slots = wb(n) // 4
        assert slots >= 2 * n and slots & (slots - 1) == 0
    assert cb(0, 5) == 0 and b"pnr_mesh_components" in err()
    assert cb(5, -1) == 0 and cb(2 ** 31, 5) == 0 and cb(5, 2 ** 31) == 0
    assert cb(5, 0) > 0 and cb(1000, 10) >= 4000
    assert lib.pnr_mesh_weld(None, 0, None, 0, None, None) == INVALID and b"pnr_mesh_weld" in err()
    assert lib.pnr_mesh_weld(None, 8, None, 0, None, None) == INVALID and b"NULL" in err()
    assert lib.pnr_mesh_components(None, 0, 0, None, 0, None, None, None, None) == INVALID
    assert b"pnr_mesh_components" in err()
    assert lib.pnr_mesh_components(None, 4, 8, None, 0, None, None, None, None) == INVALID and b"NULL" in err()
    assert lib.pnr_mesh_component_sums(None, 0, None, 0, None, None, 0, None, None) == INVALID
    assert lib.pnr_mesh_component_sums(None, 3, None, 1, None, None, 1, None, None) == INVALID and b"NULL" in err()


def test_ops_refuse_host_tensors():
    import torch

    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    for call in (lambda: ops.mesh_weld(v, f), lambda: ops.mesh_components(3, f),
                 lambda: ops.mesh_component_stats(v, f, torch.zeros(3, dtype=torch.int32),
                                                  torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(ValueError, match="HIP device"):
            call()


@pytest.mark.parametrize("name", sorted(ref.shared_meshes()))
def test_numpy_backend_matches_the_references(name):
    v, f = meshes()[name]
    remap = evaluate.weld_np(v)
    assert remap.dtype == np.int32 and np.array_equal(remap, ref.weld(v))
    wv, wf, _ = ref.weld_mesh(v, f)
    for verts, faces in ((v, f), (wv, wf)):
        vl, fl, n = evaluate.components_np(len(verts), faces)
        rv, rf, rn = ref.components(len(verts), faces)
        assert vl.dtype == fl.dtype == np.int32
        assert np.array_equal(vl, rv) and np.array_equal(fl, rf) and n == rn
        st, rs = evaluate.component_stats_np(verts, faces, vl, fl), ref.stats(verts, faces, rv, rf)
        for key in ("labels", "n_verts", "n_faces"):
            assert np.array_equal(st[key], rs[key]), key
        for key in ("area", "signed_volume"):
            bound = rs["n_faces"] * 2.0 ** -52 * rs["abs_" + key]
            assert (np.abs(st[key] - rs[key]) <= bound).all(), key


def test_weld_rules():
    v = np.array([[0.0, 1, 2], [-0.0, 1, 2], [np.nan, 0, 0], [np.nan, 0, 0], [0, 1, 2], [5, 5, 5], [0, -0.0, 0],
                  [0, 0, -0.0], [np.inf, 0, 0], [np.inf, 0, 0]], np.float32)
    assert evaluate.weld_np(v).tolist() == [0, 0, 2, 3, 0, 5, 6, 6, 8, 8]
    assert ref.weld(v).tolist() == [0, 0, 2, 3, 0, 5, 6, 6, 8, 8]
    assert evaluate.weld_np(np.zeros((0, 3), np.float32)).shape == (0,)
    sv, sf = ref.soup(*mesh_ref.icosphere(3))
    wv, wf, remap = evaluate._weld_apply_np(sv, sf)
    assert len(sv) == 3840 and len(wv) == 642 and wf.shape == sf.shape and wf.dtype == np.int32
    assert np.array_equal(wv[wf], sv[sf])          # the same triangles, record for record


def test_components_of_small_cases():
    vl, fl, n = evaluate.components_np(5, np.zeros((0, 3), np.int32))
    assert vl.tolist() == [0, 1, 2, 3, 4] and fl.shape == (0,) and n == 5
    vl, fl, n = evaluate.components_np(6, np.array([[5, 2, 4]], np.int32))
    assert vl.tolist() == [0, 1, 2, 3, 2, 2] and fl.tolist() == [2] and n == 4
    for bad in (6, -1):
        with pytest.raises(ValueError):
            evaluate.components_np(6, np.array([[0, 1, bad]], np.int32))
    sv, sf = ref.soup(*mesh_ref.icosphere(1))
    assert evaluate.components_np(len(sv), sf)[2] == 80        # a soup: one component per triangle


_SCORES = {}


def floater_scores():
    """mesh_metrics and volume_iou of icosphere(3) against itself: clean, with the floater, cleaned."""
    if not _SCORES:
        clean, dirty = ref.floater_scene()
        cv, cf, info = evaluate.clean_mesh(*dirty, keep="largest", backend="numpy")
        _SCORES["cleaned_mesh"], _SCORES["info"] = (cv, cf), info

        def score(m):
            pair = (mesh.normalize_bounds(m[0]), m[1]), (mesh.normalize_bounds(clean[0]), clean[1])
            s = evaluate.mesh_metrics(*pair, n_samples=10000, tau=0.01, backend="numpy")
            s.update(evaluate.volume_iou(*pair, n_points=5000, backend="numpy"))
            return s

        _SCORES.update(clean=score(clean), dirty=score(dirty), cleaned=score((cv, cf)))
    return _SCORES


def test_floater_scenario_cleans_to_the_clean_mesh():
    clean, dirty = ref.floater_scene()
    s = floater_scores()
    cv, cf = s["cleaned_mesh"]
    assert cv.dtype == np.float32 and cf.dtype == np.int32
    assert np.array_equal(cv, clean[0]) and np.array_equal(cf, clean[1])
    assert s["info"] == {"n_components": 2, "n_components_kept": 1, "faces_kept": 1280}
    # the soup of the same scene: welded back to 642 vertices, the sphere's triangles in their order
    sv, sf, info = evaluate.clean_mesh(*ref.soup(*dirty), keep="largest", backend="numpy")
    assert info == s["info"] and len(sv) == 642 and np.array_equal(sv[sf], clean[0][clean[1]])
    # without the weld the soup is 1,300 islands and "largest" keeps the first triangle
    _, uf, uinfo = evaluate.clean_mesh(*ref.soup(*dirty), weld=False, keep="largest", backend="numpy")
    assert uinfo == {"n_components": 1300, "n_components_kept": 1, "faces_kept": 1} and uf.tolist() == [[0, 1, 2]]


def test_floater_scenario_scores():
    """Twenty triangles out of 1,300 decide the unfiltered result; the cleaned mesh scores as the clean one."""
    s = floater_scores()
    print({k: (s["clean"][k], s["dirty"][k]) for k in ("chamfer_l1", "fscore", "normal_consistency", "iou")})
    assert s["cleaned"] == s["clean"]            # bit-identical: the arrays are equal
    assert s["clean"]["iou"] == 1.0 and s["clean"]["chamfer_l1"] < 0.03 and s["clean"]["normal_consistency"] > 0.99
    assert s["dirty"]["chamfer_l1"] > 10 * s["clean"]["chamfer_l1"]
    assert s["dirty"]["fscore"] < 0.1 * s["clean"]["fscore"]
    assert s["dirty"]["normal_consistency"] < 0.9
    assert s["dirty"]["iou"] < 0.25


def test_min_frac_and_area_on_three_spheres():
    v, f = ref.three_spheres()
    n = {"a": 1280, "b": 320, "c": 80}
    st = evaluate.component_stats_np(v, f, *evaluate.components_np(len(v), f)[:2])
    assert st["n_faces"].tolist() == [1280, 320, 80]
    assert st["area"][0] < st["area"][1] < st["area"][2]            # the face order reversed
    assert (st["signed_volume"] > 0).all()

    def kept(**kw):
        cv, cf, info = evaluate.clean_mesh(v, f, backend="numpy", **kw)
        assert info["n_components"] == 3 and info["faces_kept"] == len(cf) and cf.max() == len(cv) - 1
        return info["n_components_kept"], info["faces_kept"]

    assert kept(keep="largest") == (1, n["a"])
    assert kept(keep="largest", by="area") == (1, n["c"])
    assert kept(keep="all") == (3, 1680)
    assert kept(keep="all", min_frac=0.25) == (2, n["a"] + n["b"])     # 320 = 0.25 * 1280 stays: >=
    assert kept(keep="all", min_frac=0.26) == (1, n["a"])
    assert kept(keep="all", min_frac=1.0) == (1, n["a"])
    assert kept(keep="all", min_frac=0.0625) == (3, 1680)
    assert kept(keep="all", min_frac=0.1, by="area") == (2, n["b"] + n["c"])   # areas 0.5, 3.1, 26
    # the kept faces are the component's own triangles, in order
    cv, cf, _ = evaluate.clean_mesh(v, f, keep="largest", by="area", backend="numpy")
    assert np.array_equal(cv[cf], v[f[1600:]])
    for bad in (dict(keep="largest", min_frac=0.5), dict(keep="all", min_frac=0.0), dict(keep="all", min_frac=1.5),
                dict(keep="biggest"), dict(by="volume"), dict(backend="cuda")):
        with pytest.raises(ValueError):
            evaluate.clean_mesh(v, f, **bad)


def test_ties_go_to_the_lowest_label():
    a = mesh_ref.icosphere(1)
    v, f = ref.concat((a[0] + np.float32(4.0), a[1]), a, (a[0] - np.float32(4.0), a[1]))
    # equal face counts; the areas differ in their last bits at most, the first copy is label 0
    cv, cf, info = evaluate.clean_mesh(v, f, keep="largest", backend="numpy")
    assert info == {"n_components": 3, "n_components_kept": 1, "faces_kept": 80}
    assert np.array_equal(cv, v[:42]) and np.array_equal(cf, f[:80])
    # exact area ties: the same coordinates three times, unwelded
    v, f = ref.concat(a, a, a)
    cv, cf, info = evaluate.clean_mesh(v, f, weld=False, keep="largest", by="area", backend="numpy")
    assert info["n_components"] == 3 and np.array_equal(cf, f[:80])
    # vertex ids shuffled: the winner is the component holding the lowest vertex index
    pv, pf, perm = ref.permuted(*ref.concat((a[0] + np.float32(4.0), a[1]), a), seed=2)
    cv, cf, info = evaluate.clean_mesh(pv, pf, keep="largest", backend="numpy")
    vl = ref.components(len(pv), pf)[0]
    assert info["faces_kept"] == 80 and np.array_equal(cv, pv[vl == 0])


def test_empty_and_faceless_meshes():
    e = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    for m in (e, (np.ones((4, 3), np.float32), e[1])):
        cv, cf, info = evaluate.clean_mesh(*m, backend="numpy")
        assert cv.shape == (0, 3) and cf.shape == (0, 3) and cf.dtype == np.int32
        assert info == {"n_components": 0, "n_components_kept": 0, "faces_kept": 0}


# ---- scripts/eval_mesh.py ----------------------------------------------------------------------------
def test_eval_mesh_script_components(tmp_path):
    """Two objects, the prediction of "b" with a far floater (index units).  Default flags: the files of
    the parent's code path (the surface lines only, "b" ruined).  --components largest: the three
    lines follow, "b" scores as "a" does, and the reduce averages the counts."""
    res, n = 33, 1500
    out, gt = mesh_ref.write_eval_tree(str(tmp_path), res, {"a": (0.5, 1.0), "b": (0.5, 1.0)})
    v, f = mesh_ref.icosphere(3, 0.5)
    fv, ff = mesh_ref.icosphere(0, 0.01)
    dv, df = ref.concat((v, f), (fv + np.array([0.95, 0, 0], np.float32), ff))
    mesh.write_stl(os.path.join(out, "b", "b_mesh.stl"), mesh_ref.to_index_units(dv, res), df)
    cmd = [sys.executable, os.path.join(REPO, "scripts", "eval_mesh.py"), "-O", out, "-G", gt, "--mesh_res", str(res),
           "--n_samples", str(n), "--tau", "0.05", "--seed", "5", "--metrics_backend", "numpy"]
    r = _run(cmd)
    assert r.returncode == 0, r.stderr[-3000:]
    old = {k: open(os.path.join(out, k, "mesh_metrics.txt")).read() for k in ("a", "b")}
    old_all = open(os.path.join(out, "all_mesh_metrics.txt")).read()
    # the parent's code path, restated: read, map to the world, normalise both, score, write
    for k in ("a", "b"):
        pv, pf = mesh.read_stl_indexed(os.path.join(out, k, k + "_mesh.stl"))
        gv, gf = mesh.read_stl_indexed(os.path.join(gt, k + ".stl"))
        pv = pv * (2.0 / (res - 1)) - 1.0
        s = evaluate.mesh_metrics((mesh.normalize_bounds(pv), pf), (mesh.normalize_bounds(gv), gf), n_samples=n,
                                  tau=0.05, seed=5, backend="numpy")
        assert old[k] == "".join("{} {!r}\n".format(name, float(s[name])) for name in evaluate.MESH_METRIC_NAMES)
    plain = {k: {r[0]: float(r[1]) for r in _lines(os.path.join(out, k, "mesh_metrics.txt"))} for k in ("a", "b")}
    assert plain["b"]["chamfer_l1"] > 5 * plain["a"]["chamfer_l1"]
    # the flag on files written without it: the reduce names the object and stops
    r = _run(cmd + ["--components", "largest", "-R"])
    assert r.returncode != 0 and "object a" in r.stderr and "component" in r.stderr
    assert open(os.path.join(out, "all_mesh_metrics.txt")).read() == old_all
    # the conflict and a bad fraction are rejected before anything runs
    for extra in (["--components", "largest", "--min_component_frac", "0.5"], ["--min_component_frac", "0"],
                  ["--min_component_frac", "1.5"]):
        r = _run(cmd + extra)
        assert r.returncode != 0 and "min_component_frac" in r.stderr
    r = _run(cmd + ["--components", "largest", "--overwrite"])
    assert r.returncode == 0, r.stderr[-3000:]
    names = list(evaluate.MESH_METRIC_NAMES) + list(evaluate.CLEAN_INFO_NAMES)
    vals = {}
    for k in ("a", "b"):
        rows = _lines(os.path.join(out, k, "mesh_metrics.txt"))
        assert [r[0] for r in rows] == names
        vals[k] = {r[0]: float(r[1]) for r in rows}
    assert open(os.path.join(out, "a", "mesh_metrics.txt")).read().startswith(old["a"])   # one component: unchanged
    assert [vals["a"][k] for k in evaluate.CLEAN_INFO_NAMES] == [1.0, 1.0, 1280.0]
    assert [vals["b"][k] for k in evaluate.CLEAN_INFO_NAMES] == [2.0, 1.0, 1280.0]
    # "b" cleaned is "a"'s welded sphere, vertex for vertex: the same scores to the bit
    assert all(vals["b"][k] == vals["a"][k] for k in evaluate.MESH_METRIC_NAMES)
    rows = _lines(os.path.join(out, "all_mesh_metrics.txt"))
    assert [r[0] for r in rows] == names + ["objects"] and rows[-1][1] == "2"
    for name, val in rows[:-1]:
        assert float(val) == (0.0 + vals["a"][name] + vals["b"][name]) / 2
    # --min_component_frac keeps the floater out too (20 < 0.5 * 1280), and in with a small fraction
    for frac, kept in (("0.5", [2.0, 1.0, 1280.0]), ("0.01", [2.0, 2.0, 1300.0])):
        r = _run(cmd + ["--min_component_frac", frac, "--overwrite"])
        assert r.returncode == 0, r.stderr[-3000:]
        got = {r[0]: float(r[1]) for r in _lines(os.path.join(out, "b", "mesh_metrics.txt"))}
        assert [got[k] for k in evaluate.CLEAN_INFO_NAMES] == kept
    # mixing: "a" rewritten without the flag, "b" with it -> the reduce stops at "a"
    os.remove(os.path.join(out, "a", "mesh_metrics.txt"))
    r = _run(cmd)
    assert r.returncode == 0, r.stderr[-3000:]
    r = _run(cmd + ["--components", "largest", "-R"])
    assert r.returncode != 0 and "object a" in r.stderr
    # and with the defaults again: byte for byte the first run's files
    r = _run(cmd + ["--overwrite"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert {k: open(os.path.join(out, k, "mesh_metrics.txt")).read() for k in ("a", "b")} == old
    assert open(os.path.join(out, "all_mesh_metrics.txt")).read() == old_all
