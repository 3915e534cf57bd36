"""Yardstick of the mesh-rendering tests (a helper, not a conftest): include/pnr_abi.h, "Mesh
rendering", restated in numpy twice, sharing no code with pnr.evaluate.

  cast64    a brute-force ray cast in fp64 on the fp32 inputs: Moeller-Trumbore with inclusive bounds
            over all rays x faces, the rays those of gen_rays (origin pose[:3, 3], direction
            R normalize((i - cx) / fx, -(j - cy) / fy, -1)).  The reference of every comparison.
  sure      the pixels a test may judge: the rays through (i +- delta, j +- delta), delta = 1/64 pixel,
            agree with the centre ray on hit / miss and their four depths are within 1 % of its.
  raster32  the header's per-(pixel, face) rule operation by operation in fp32, fmas where the header
            puts them (an fp32 fma is the fp64 product-sum of fp32 values rounded to fp32), over all
            pixels x faces: the host emulation of the device arithmetic.

A face with an index outside [0, V), a non-finite vertex or zero area contributes nothing in both."""
import numpy as np

F32, F64 = np.float32, np.float64
DELTA = 1.0 / 64.0


def cam(width, height, focal, c=None):
    """(fx, fy, cx, cy) as fp32-representable floats."""
    fx, fy = (focal, focal) if np.isscalar(focal) else focal
    cx, cy = (width * 0.5, height * 0.5) if c is None else ((c, c) if np.isscalar(c) else c)
    return tuple(float(F32(t)) for t in (fx, fy, cx, cy))


def rays64(pose, width, height, fx, fy, cx, cy, di=0.0, dj=0.0):
    """(origin (3,), unit directions (H W, 3)) of one view in fp64, the pixels moved by (di, dj)."""
    pose = np.asarray(pose, F32).astype(F64)
    jj, ii = np.meshgrid(np.arange(height, dtype=F64) + dj, np.arange(width, dtype=F64) + di, indexing="ij")
    u = np.stack([(ii - cx) / fx, -(jj - cy) / fy, -np.ones_like(ii)], -1).reshape(-1, 3)
    u /= np.sqrt((u * u).sum(-1, keepdims=True))
    return pose[:3, 3], u @ pose[:3, :3].T


def good_faces(v, f):
    """Indices of the faces that take part: indices in range, finite vertices, a non-zero area."""
    v = np.asarray(v, F32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    ids = np.nonzero(ok)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        tri = v[f[ids]]
        u, w = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]      # fp32, unfused: the header's zero-area rule
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                      u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)
        keep = np.isfinite(tri).all((1, 2)) & (n != 0).any(1) & np.isfinite(n).all(1)
    return ids[keep]


def moller_trumbore(o, d, tri):
    """(u, v, t) of rays (P, 3) against triangles (T, 3, 3), each (P, T), fp64; NaN where det is 0."""
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    pvec = np.cross(d[:, None, :], e2[None, :, :])
    det = (e1[None] * pvec).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = np.where(det != 0, 1.0 / det, np.nan)
        tvec = (o - a)[None]
        u = (tvec * pvec).sum(-1) * inv
        qvec = np.cross(tvec, e1[None])
        v = (d[:, None, :] * qvec).sum(-1) * inv
        t = (e2[None] * qvec).sum(-1) * inv
    return u, v, t


def _cast_view(pose, v64, f, ids, width, height, k, di=0.0, dj=0.0, slack=0.0, chunk=None):
    o, d = rays64(pose, width, height, *k, di=di, dj=dj)
    n = len(d)
    face, depth = np.full(n, -1, np.int64), np.zeros(n)
    if len(ids) == 0 or not np.isfinite(np.asarray(pose, F64)[:3]).all():
        return face, depth
    tri = v64[f[ids]]
    chunk = chunk or max(1, (1 << 20) // len(ids))
    for i in range(0, n, chunk):
        u, w, t = moller_trumbore(o, d[i:i + chunk], tri)
        with np.errstate(invalid="ignore"):
            hit = (u >= -slack) & (w >= -slack) & (u + w <= 1.0 + slack) & (t > 0)
        t = np.where(hit, t, np.inf)
        best = t.argmin(1)
        tb = t[np.arange(len(best)), best]
        got = np.isfinite(tb)
        face[i:i + chunk] = np.where(got, ids[best], -1)
        depth[i:i + chunk] = np.where(got, tb, 0.0)
    return face, depth


def cast64(v, f, poses, width, height, focal, c=None, di=0.0, dj=0.0):
    """(face (NV, H, W) int64, depth (NV, H, W) fp64): the nearest inclusive hit with t > 0, the lowest
    face among equal depths; -1 / 0 where there is none."""
    k = cam(width, height, focal, c)
    v64 = np.asarray(v, F32).reshape(-1, 3).astype(F64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ids = good_faces(v, f)
    out = [_cast_view(p, v64, f, ids, width, height, k, di, dj) for p in np.asarray(poses, F32)]
    shape = (len(out), height, width)
    return np.stack([a for a, _ in out]).reshape(shape), np.stack([b for _, b in out]).reshape(shape)


def sure(v, f, poses, width, height, focal, c=None, centre=None):
    """bool (NV, H, W): the pixels whose four neighbours at +-DELTA agree with the centre ray."""
    face0, depth0 = centre if centre is not None else cast64(v, f, poses, width, height, focal, c)
    ok = np.ones(face0.shape, bool)
    for di in (-DELTA, DELTA):
        for dj in (-DELTA, DELTA):
            face, depth = cast64(v, f, poses, width, height, focal, c, di, dj)
            ok &= (face >= 0) == (face0 >= 0)
            ok &= np.abs(depth - depth0) <= 0.01 * depth0
    return ok


def face_answers(v, f, poses, width, height, focal, face, c=None):
    """For a returned face per pixel (NV, H, W; -1 allowed): (inside (NV, H, W) bool, t (NV, H, W)) of
    THAT face against the pixel's ray in fp64, inside with a barycentric slack of 1e-4."""
    k = cam(width, height, focal, c)
    v64 = np.asarray(v, F32).reshape(-1, 3).astype(F64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    face = np.asarray(face, np.int64)
    inside, t_out = np.zeros(face.shape, bool), np.zeros(face.shape)
    for n, p in enumerate(np.asarray(poses, F32)):
        o, d = rays64(p, width, height, *k)
        fl = face[n].reshape(-1)
        m = fl >= 0
        if not m.any():
            continue
        tri = v64[f[fl[m]]]
        a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        pvec = np.cross(d[m], e2)
        det = (e1 * pvec).sum(-1)
        tvec = o - a
        u = (tvec * pvec).sum(-1) / det
        qvec = np.cross(tvec, e1)
        w = (d[m] * qvec).sum(-1) / det
        t = (e2 * qvec).sum(-1) / det
        ins = np.zeros(len(fl), bool)
        ins[m] = (u >= -1e-4) & (w >= -1e-4) & (u + w <= 1.0 + 1e-4) & (t > 0)
        tt = np.zeros(len(fl))
        tt[m] = t
        inside[n], t_out[n] = ins.reshape(face[n].shape), tt.reshape(face[n].shape)
    return inside, t_out


# ---- the device arithmetic in fp32 -----------------------------------------------------------------
def _fma(a, b, c):
    a, b, c = (np.asarray(t, F32).astype(F64) for t in (a, b, c))
    return (a * b + c).astype(F32)


def _lex_less(p, q):
    return np.where(p[:, 0] != q[:, 0], p[:, 0] < q[:, 0],
                    np.where(p[:, 1] != q[:, 1], p[:, 1] < q[:, 1], p[:, 2] < q[:, 2]))


def _edge_normal(pw, qw, pc, qc):
    swap = _lex_less(qw, pw)[:, None]
    lo, hi = np.where(swap, qc, pc), np.where(swap, pc, qc)
    e = hi - lo
    n = np.stack([lo[:, 1] * e[:, 2] - lo[:, 2] * e[:, 1], lo[:, 2] * e[:, 0] - lo[:, 0] * e[:, 2],
                  lo[:, 0] * e[:, 1] - lo[:, 1] * e[:, 0]], -1)
    assert n.dtype == F32
    return np.where(swap, -n, n)


def pixel_dirs32(width, height, fx, fy, cx, cy):
    """(X, -Y, |u|) of every pixel in fp32, (H W,) each, as pnr_gen_rays rounds them."""
    fx, fy, cx, cy = (F32(t) for t in (fx, fy, cx, cy))
    jj, ii = np.meshgrid(np.arange(height, dtype=F32), np.arange(width, dtype=F32), indexing="ij")
    X, Yn = ((ii - cx) / fx).reshape(-1), (-((jj - cy) / fy)).reshape(-1)
    length = np.sqrt((X * X + Yn * Yn) + F32(1.0))
    assert X.dtype == Yn.dtype == length.dtype == F32
    return X, Yn, length


def raster32(v, f, poses, width, height, focal, c=None):
    """(face (NV, H, W) int64, depth (NV, H, W) fp32) by the header's fp32 rule over all pixels x faces:
    what the device computes, bit for bit up to the double rounding of the emulated fmas."""
    k = cam(width, height, focal, c)
    v = np.asarray(v, F32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ids = good_faces(v, f)
    X, Yn, length = pixel_dirs32(width, height, *k)
    poses = np.asarray(poses, F32)
    face, depth = np.full((len(poses), len(X)), -1, np.int64), np.zeros((len(poses), len(X)), F32)
    for n, pose in enumerate(poses):
        if len(ids) == 0 or not np.isfinite(pose[:3]).all():
            continue
        R, o = pose[:3, :3], pose[:3, 3]
        w = [v[f[ids, j]] for j in range(3)]
        cs = []
        for p in w:
            d = p - o
            cs.append(np.stack([_fma(R[2, a], d[:, 2], _fma(R[1, a], d[:, 1], R[0, a] * d[:, 0])) for a in range(3)], -1))
        front = ~((cs[0][:, 2] >= 0) & (cs[1][:, 2] >= 0) & (cs[2][:, 2] >= 0))
        n_ab, n_bc, n_ca = (_edge_normal(w[0], w[1], cs[0], cs[1]), _edge_normal(w[1], w[2], cs[1], cs[2]),
                            _edge_normal(w[2], w[0], cs[2], cs[0]))
        x, y = X[:, None], Yn[:, None]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            e_ab = _fma(n_ab[:, 0], x, _fma(n_ab[:, 1], y, -n_ab[:, 2]))
            e_bc = _fma(n_bc[:, 0], x, _fma(n_bc[:, 1], y, -n_bc[:, 2]))
            e_ca = _fma(n_ca[:, 0], x, _fma(n_ca[:, 1], y, -n_ca[:, 2]))
            pos = (e_ab > 0) | (e_bc > 0) | (e_ca > 0)
            neg = (e_ab < 0) | (e_bc < 0) | (e_ca < 0)
            det = (e_ab + e_bc) + e_ca
            num = _fma(e_ca, cs[1][:, 2], _fma(e_bc, cs[0][:, 2], e_ab * cs[2][:, 2]))
            s = -(num / det)
            assert s.dtype == F32
            hit = ~(pos & neg) & (det != 0) & (s > 0) & np.isfinite(s) & front
        s = np.where(hit, s, F32(np.inf))
        best = s.argmin(1)
        sb = s[np.arange(len(best)), best]
        got = np.isfinite(sb)
        face[n] = np.where(got, ids[best], -1)
        depth[n] = np.where(got, sb * length, F32(0.0))
    shape = (len(poses), height, width)
    return face.reshape(shape), depth.reshape(shape)


# ---- meshes and cameras of the tests -----------------------------------------------------------------
def golden_poses(n_views, radius):
    """The golden-spiral cameras restated: 2 n points, the upper half, looking at the origin, z up;
    (n, 4, 4) float32 in the loader's convention."""
    n = 2 * n_views
    out = np.zeros((n_views, 4, 4))
    g = (1 + 5 ** 0.5) / 2
    for i in range(n_views):
        theta, phi = 2 * np.pi * i / g, np.arccos(1 - 2 * (i + 0.5) / n)
        pos = radius * np.array([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)])
        z = pos / np.linalg.norm(pos)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        out[i, :3, 0], out[i, :3, 1], out[i, :3, 2], out[i, :3, 3], out[i, 3, 3] = x, np.cross(z, x), z, pos, 1.0
    return out.astype(F32)


def sphere_with_floater(subdivisions):
    """icosphere(subdivisions) * 0.45 plus an icosphere(1) * 0.12 floater at (0.5, 0.1, 0.2)."""
    import mesh_ref

    v0, f0 = mesh_ref.icosphere(subdivisions, 0.45)
    v1, f1 = mesh_ref.icosphere(1, 0.12)
    v = np.concatenate([v0, v1 + np.array([0.5, 0.1, 0.2], F32)]).astype(F32)
    return v, np.concatenate([f0, f1 + len(v0)]).astype(np.int32)


CASES = {"A": dict(subdivisions=2, n_views=4, radius=1.3, size=32, focal=32.8125, c=16.0),
         "B": dict(subdivisions=3, n_views=4, radius=1.3, size=48, focal=49.2, c=24.0)}
_case_cache = {}


def case(name):
    """The parity case `name` with its fp64 cast and sure mask, computed once and shared: a dict with v, f,
    poses, size, focal, c, face64, depth64, sure.  Callers must not modify the arrays."""
    if name not in _case_cache:
        k = CASES[name]
        v, f = sphere_with_floater(k["subdivisions"])
        poses = golden_poses(k["n_views"], k["radius"])
        face64, depth64 = cast64(v, f, poses, k["size"], k["size"], k["focal"], k["c"])
        ok = sure(v, f, poses, k["size"], k["size"], k["focal"], k["c"], centre=(face64, depth64))
        _case_cache[name] = dict(v=v, f=f, poses=poses, size=k["size"], focal=k["focal"], c=k["c"], face64=face64,
                                 depth64=depth64, sure=ok)
    return _case_cache[name]


def plane_quads(step, size=17, f=16.0, c=8.0, soup=False):
    """The plane z = -1 tiled by quads of `step` pixels over a size x size image of a camera at the origin
    with fx = fy = f, cx = cy = c: vertex (p, q) at ((p step - c) / f, -(q step - c) / f, -1), every value a
    short dyadic number.  Each quad is the faces (v00, v10, v11) and (v00, v11, v01).  `soup`: unwelded."""
    n = (size - 1) // step
    g = np.arange(n + 1, dtype=F64) * step
    px, py = np.meshgrid((g - c) / f, -(g - c) / f, indexing="xy")            # [q, p]
    v = np.stack([px, py, -np.ones_like(px)], -1).reshape(-1, 3).astype(F32)
    idx = lambda p, q: q * (n + 1) + p   # noqa: E731
    faces = []
    for q in range(n):
        for p in range(n):
            faces += [[idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)], [idx(p, q), idx(p + 1, q + 1), idx(p, q + 1)]]
    faces = np.asarray(faces, np.int32)
    if soup:
        v = v[faces.reshape(-1)]
        faces = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return v, faces


def lowest_containing_face(v, f, width, height, fx, fy, cx, cy):
    """For the camera at the origin looking down -z: (H, W) int64, the lowest face whose inclusive
    Moeller-Trumbore test contains each pixel's ray (-1 if none).  Exact for dyadic inputs."""
    jj, ii = np.meshgrid(np.arange(height, dtype=F64), np.arange(width, dtype=F64), indexing="ij")
    d = np.stack([(ii - cx) / fx, -(jj - cy) / fy, -np.ones_like(ii)], -1).reshape(-1, 3)   # unnormalised: exact
    tri = np.asarray(v, F32).astype(F64)[np.asarray(f, np.int64)]
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    pvec = np.cross(d[:, None, :], e2[None])
    det = (e1[None] * pvec).sum(-1)
    sg = np.sign(det)
    tvec = -a[None]                                                          # the origin is the camera
    un = sg * (tvec * pvec).sum(-1)
    qvec = np.cross(tvec, e1[None])
    wn = sg * (d[:, None, :] * qvec).sum(-1)
    tn = sg * (e2[None] * qvec).sum(-1)
    hit = (det != 0) & (un >= 0) & (wn >= 0) & (un + wn <= np.abs(det)) & (tn > 0)          # no division
    first = hit.argmax(1)
    return np.where(hit.any(1), first, -1).reshape(height, width)


def box_mesh(h=0.5):
    """The 12 faces of the cube [-h, h]^3, outward winding."""
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], F32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f
