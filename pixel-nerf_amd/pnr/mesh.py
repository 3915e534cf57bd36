"""Mesh files of the reference's two exporters, without trimesh / PyMCubes: binary STL
(eval/eval.py:106-108 exports a trimesh.Trimesh to ``<object>_mesh.stl``) and the OBJ of
src/util/recon.py:81-106."""
import numpy as np


def _np(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


_STL_REC = np.dtype([("normal", "<f4", (3,)), ("tri", "<f4", (3, 3)), ("attr", "<u2")])


def write_stl(path, verts, faces):
    """Binary STL: an 80-byte header, a uint32 triangle count, one 50-byte record per triangle
    (unit facet normal by the right-hand rule from the geometry, (0, 0, 0) for a zero-area facet;
    the three float32 vertices; a zero attribute word).  An empty mesh is a valid 84-byte file."""
    v = _np(verts, np.float32).reshape(-1, 3)
    f = _np(faces, np.int64).reshape(-1, 3)
    rec = np.zeros(f.shape[0], _STL_REC)
    if f.shape[0]:
        tri = v[f]
        n = np.cross((tri[:, 1] - tri[:, 0]).astype(np.float64), (tri[:, 2] - tri[:, 0]).astype(np.float64))
        ln = np.sqrt((n * n).sum(-1, keepdims=True))
        rec["normal"] = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0).astype(np.float32)
        rec["tri"] = tri
    with open(path, "wb") as fh:
        fh.write(b"pnr binary STL".ljust(80, b" "))
        fh.write(np.uint32(f.shape[0]).tobytes())
        fh.write(rec.tobytes())


def read_stl(path):
    """(normals (T, 3), triangles (T, 3, 3)) float32 of a binary STL."""
    with open(path, "rb") as fh:
        raw = fh.read()
    n = int(np.frombuffer(raw, "<u4", 1, 80)[0])
    if len(raw) != 84 + 50 * n:
        raise ValueError("%s: %d bytes, a binary STL of %d triangles has %d" % (path, len(raw), n, 84 + 50 * n))
    rec = np.frombuffer(raw, _STL_REC, n, 84)
    return rec["normal"].copy(), rec["tri"].copy()


def read_stl_indexed(path):
    """(verts (3 T, 3) float32, faces (T, 3) int32) of a binary STL: the triangle soup as it stands,
    ``faces = arange(3 T).reshape(T, 3)`` (no vertex is merged; surface sampling needs none)."""
    _, tris = read_stl(path)
    verts = np.ascontiguousarray(tris.reshape(-1, 3), dtype=np.float32)
    return verts, np.arange(verts.shape[0], dtype=np.int32).reshape(-1, 3)


def normalize_bounds(verts, radius=1.0):
    """Vertices moved so that the centre of their bounding box is the origin and scaled so that the
    farthest one lies at ``radius``: what the fork's Blender step does to a ground-truth STL before it
    renders the views.  Works on numpy arrays and torch tensors alike (same type and device back); an
    empty or single-point set is only centred."""
    if len(verts) == 0:
        return verts
    if hasattr(verts, "detach"):
        centre = 0.5 * (verts.min(0).values + verts.max(0).values)
        v = verts - centre
        far = v.norm(dim=1).max()
        return v * (radius / far) if float(far) > 0.0 else v
    v = np.asarray(verts)
    v = v - 0.5 * (v.min(0) + v.max(0))
    far = np.sqrt((v.astype(np.float64) ** 2).sum(1)).max()
    return (v * (radius / far)).astype(v.dtype) if far > 0.0 else v


def save_obj(vertices, triangles, path, vert_rgb=None):
    """OBJ with optional vertex colours, the reference's format (recon.py:81-106): ``v`` lines with
    %.4f coordinates (and colours), ``f`` lines with 1-based indices."""
    vertices = _np(vertices, np.float64)
    triangles = _np(triangles, np.int64)
    with open(path, "w") as file:
        if vert_rgb is None:
            for v in vertices:
                file.write("v %.4f %.4f %.4f\n" % (v[0], v[1], v[2]))
        else:
            vert_rgb = _np(vert_rgb, np.float64)
            for idx, v in enumerate(vertices):
                c = vert_rgb[idx]
                file.write("v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (v[0], v[1], v[2], c[0], c[1], c[2]))
        for f in triangles:
            file.write("f %d %d %d\n" % (f[0] + 1, f[1] + 1, f[2] + 1))
