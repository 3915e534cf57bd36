"""pnr.mesh (binary STL, the reference's OBJ) and the host-side refusals of the isosurface ABI:
no GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from pnr import _lib, mesh, ops


def test_stl_layout_and_normals(tmp_path):
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [5, 5, 5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 1], [0, 3, 1], [4, 4, 4], [0, 1, 1]], np.int32)
    path = str(tmp_path / "m.stl")
    mesh.write_stl(path, torch.from_numpy(verts), torch.from_numpy(faces))
    raw = open(path, "rb").read()
    assert len(raw) == 84 + 50 * 5
    assert np.frombuffer(raw, "<u4", 1, 80)[0] == 5
    rec = raw[84:84 + 50]
    assert np.array_equal(np.frombuffer(rec, "<f4", 12), np.array([0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 2, 0], np.float32))
    assert rec[48:] == b"\0\0"
    normals, tris = mesh.read_stl(path)
    assert np.array_equal(tris, verts[faces])
    assert np.array_equal(normals, np.array([[0, 0, 1], [0, 0, -1], [0, 1, 0], [0, 0, 0], [0, 0, 0]], np.float32))
    mesh.write_stl(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert len(open(path, "rb").read()) == 84 and len(mesh.read_stl(path)[1]) == 0
    with open(path, "ab") as f:
        f.write(b"x")
    with pytest.raises(ValueError):
        mesh.read_stl(path)


def test_save_obj_is_the_reference_format(tmp_path):
    v = np.array([[0.125, -1, 2], [3, 4, 5.75]])
    t = np.array([[0, 1, 1]])
    mesh.save_obj(v, t, str(tmp_path / "a.obj"))
    assert (tmp_path / "a.obj").read_text() == "v 0.1250 -1.0000 2.0000\nv 3.0000 4.0000 5.7500\nf 1 2 2\n"
    mesh.save_obj(v, t, str(tmp_path / "b.obj"), vert_rgb=np.array([[1, 0, 0.5], [0, 1, 0.25]]))
    assert (tmp_path / "b.obj").read_text().splitlines()[1] == "v %.4f %.4f %.4f 0.0000 1.0000 0.2500" % tuple(v[1])


def test_isosurface_abi_refuses_without_touching_a_device():
    lib = _lib.load()
    assert lib.pnr_mc_workspace_bytes(1025, 2, 2) == 0 and lib.pnr_mc_workspace_bytes(2, 0, 2) == 0
    n = lib.pnr_mc_workspace_bytes(256, 256, 256)
    assert 12 * 256 ** 3 <= n <= 12 * 256 ** 3 + (1 << 20)
    assert lib.pnr_mc_workspace_bytes(1024, 1024, 1024) >= 12 * 1024 ** 3
    assert lib.pnr_mc_count(None, 2, 2, 2, 0.0, None, 0, None, None) == -1 and b"NULL" in lib.pnr_last_error()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    assert lib.pnr_mc_count(p, 1025, 2, 2, 0.0, p, 4096, p, None) == -2 and b"1024" in lib.pnr_last_error()
    assert lib.pnr_mc_count(p, 0, 2, 2, 0.0, p, 4096, p, None) == -1
    assert lib.pnr_mc_count(p, 2, 2, 2, 0.0, p, 8, p, None) == -4
    assert lib.pnr_mc_count(p, 2, 2, 2, 0.0, ctypes.c_void_p(p.value + 4), 4096, p, None) == -1
    assert b"aligned" in lib.pnr_last_error()
    assert lib.pnr_mc_emit(p, 2, 2, 2, 0.0, p, 4096, None, 3, None, 0, None) == -1
    assert lib.pnr_mc_emit(p, 2, 2, 2, 0.0, p, 4096, p, -1, p, 0, None) == -1
    assert lib.pnr_mc_emit(p, 2, 2, 2, 0.0, p, 4096, p, 2 ** 31, p, 0, None) == -1
    assert lib.pnr_mc_emit(p, 2048, 2, 2, 0.0, p, 4096, p, 1, p, 1, None) == -2
    assert lib.pnr_mc_case_table(None) == -1
    with pytest.raises(ValueError):
        ops.marching_cubes(torch.zeros(3, 3, 3), 0.0)       # a CPU tensor: no fallback
