"""Host restatements of the device mesh rules, in numpy (include/pnr_abi.h: "Mesh metrics", "Mesh
containment", "Mesh cleanup", "Mesh rendering").

Every function here states on the host what one pnr.ops mesh wrapper computes on the device, from
the same fp32 inputs and with the same draws: the ``numpy`` backends of pnr.evaluate are assembled
from them, and the GPU tests compare the device against them.  tests/*_ref.py restate the same rules
once more, independently, as the yardstick for this module.
"""
import numpy as np
import torch

_RNG_MESH = 4     # PNR_RNG_MESH
_RNG_VOLUME = 5   # PNR_RNG_VOLUME


def _philox_uniform(seed, stream, count):
    """(count,) float32: U[0, 1) of elements e = 0 .. count - 1 of a counter-mode stream
    (include/pnr_abi.h pnr_rng: Philox4x32-10, counter (lo32 e, hi32 e, stream, 0), key = seed,
    (word 0 >> 8) * 2^-24)."""
    mask = np.uint64(0xFFFFFFFF)
    e = np.arange(count, dtype=np.uint64)
    c = [e & mask, e >> np.uint64(32), np.full(count, stream, np.uint64), np.zeros(count, np.uint64)]
    k = [np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)]
    for r in range(10):
        if r:
            k = [(k[0] + np.uint64(0x9E3779B9)) & mask, (k[1] + np.uint64(0xBB67AE85)) & mask]
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
    return (c[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _draws(seed, stream, n):
    """(n, 3) float32: draws 0 .. 2 of rays 0 .. n - 1 of a counter-mode stream of width 3 at offset 0
    (element e = 3 ray + k), what pnr_mesh_sample (_RNG_MESH) and pnr_box_sample (_RNG_VOLUME) draw on
    the device."""
    return _philox_uniform(seed, stream, 3 * n).reshape(n, 3)


def _host_mesh(verts, faces, index=np.int64):
    """A mesh of tensors or arrays as contiguous arrays: verts (V, 3) float32, faces (T, 3) ``index``."""
    v, f = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (verts, faces))
    return np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, index).reshape(-1, 3)


def sample_mesh_np(verts, faces, n, seed=0):
    """pnr_mesh_sample's rule on the host: ``(points (n, 3) float32, normals (n, 3) float32, tri (n,)
    int32, total area)``.  Areas in fp64 from the fp32 vertices, their inclusive sum with np.cumsum,
    the first face whose sum exceeds u0 * total, the fold of (u1, u2) at u1 + u2 > 1, the point
    a + u1 (b - a) + u2 (c - a) in fp32.  The device's sum runs in another fixed order, so a sample
    whose target lies within rounding of a face boundary may fall on the neighbouring face there."""
    v, f = _host_mesh(verts, faces)
    if f.shape[0] == 0 or f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError("sample_mesh_np: no faces, or a face index outside [0, %d)" % v.shape[0])
    a, b, c = (v[f[:, i]] for i in range(3))
    cr = np.cross(b.astype(np.float64) - a, c.astype(np.float64) - a)
    ln = np.sqrt(cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1] + cr[:, 2] * cr[:, 2])
    cdf = np.cumsum(0.5 * ln)
    total = float(cdf[-1])
    if not (total > 0.0 and np.isfinite(total)):
        raise ValueError("sample_mesh_np: the total area is %r, nothing to sample" % total)
    u = _draws(seed, _RNG_MESH, n)
    tri = np.minimum(np.searchsorted(cdf, u[:, 0].astype(np.float64) * total, side="right"), len(cdf) - 1)
    u1, u2 = u[:, 1].copy(), u[:, 2].copy()
    fold = (u1 + u2) > np.float32(1.0)
    u1[fold], u2[fold] = np.float32(1.0) - u1[fold], np.float32(1.0) - u2[fold]
    pa, pb, pc = a[tri], b[tri], c[tri]
    points = (pa + u1[:, None] * (pb - pa)) + u2[:, None] * (pc - pa)
    normals = (cr[tri] / ln[tri][:, None]).astype(np.float32)
    return points.astype(np.float32), normals, tri.astype(np.int32), total


def nearest_np(a, b, chunk=2048):
    """(squared distance, index) of the nearest row of b for every row of a, in fp64 on the host:
    scipy's cKDTree where scipy imports, a chunked brute force otherwise."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        d, idx = cKDTree(b).query(a)
        return d * d, idx.astype(np.int64)
    d2 = np.empty(len(a))
    idx = np.empty(len(a), np.int64)
    for i in range(0, len(a), chunk):
        dd = ((a[i:i + chunk, None, :] - b[None, :, :]) ** 2).sum(-1)
        idx[i:i + chunk] = dd.argmin(1)
        d2[i:i + chunk] = dd[np.arange(dd.shape[0]), idx[i:i + chunk]]
    return d2, idx


def box_sample_np(lo, hi, n, seed=0):
    """pnr_box_sample's rule on the host: (n, 3) float32, coordinate k = u_k * fl(hi_k - lo_k) + lo_k
    with one rounding.  The product is exact in fp64 and the sum is rounded there before it is
    rounded to fp32, so a coordinate differs from the device's fma by one ulp where the fp64 sum
    lands on an fp32 tie (about 2^-29 of the draws)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ext = (hi - lo).astype(np.float64)
    return (_draws(seed, _RNG_VOLUME, n).astype(np.float64) * ext + lo.astype(np.float64)).astype(np.float32)


def winding_np(verts, faces, points, chunk=None):
    """Generalized winding number on the host, (n,) float64: pnr_winding's formula (include/pnr_abi.h,
    "Mesh containment") in fp64 numpy on the fp32 inputs, ``chunk`` queries at a time (default: about
    2^21 pairs per step).  A face with an index outside [0, V) contributes 0."""
    v, f = _host_mesh(verts, faces)
    v = v.astype(np.float64)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    f = f[((f >= 0) & (f < len(v))).all(1)]
    w = np.zeros(len(p))
    if len(f) == 0 or len(p) == 0:
        return w
    tri = [v[f[:, k], c][None, :] for k in range(3) for c in range(3)]   # Ax Ay Az Bx ... Cz, each (1, T)
    if chunk is None:
        chunk = max(1, (1 << 21) // len(f))
    with np.errstate(invalid="ignore"):
        for i in range(0, len(p), chunk):
            q = [p[i:i + chunk, c, None] for c in range(3)]
            ax, ay, az, bx, by, bz, cx, cy, cz = (tri[3 * k + c] - q[c] for k in range(3) for c in range(3))
            la = np.sqrt(ax * ax + ay * ay + az * az)
            lb = np.sqrt(bx * bx + by * by + bz * bz)
            lc = np.sqrt(cx * cx + cy * cy + cz * cz)
            num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
            den = (la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la
                   + (cx * ax + cy * ay + cz * az) * lb)
            w[i:i + chunk] = (2.0 * np.arctan2(num, den)).sum(-1) / (4.0 * np.pi)   # arctan2(0, 0) = 0
    return w


def _signed_volume_np(v, f):
    """Sum of a . (b x c) / 6 over the faces, fp64: negative for a mesh whose faces look inwards."""
    t = np.asarray(v, np.float64)[np.asarray(f, np.int64)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def weld_np(verts):
    """pnr_mesh_weld's rule on the host (include/pnr_abi.h, "Mesh cleanup"): ``remap (V,) int32``,
    remap[i] = the lowest index whose three coordinates compare equal to vertex i's as floats (-0.0
    equals +0.0); a vertex with a NaN coordinate keeps remap[i] = i.  A lexicographic sort, then the
    minimum index of every run of equal rows."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    remap = np.arange(v.shape[0], dtype=np.int64)
    ok = np.nonzero(~np.isnan(v).any(1))[0]
    if ok.size:
        w = v[ok] + np.float32(0.0)   # -0 + 0 = +0: equal floats sort next to each other either way
        order = np.lexsort((w[:, 2], w[:, 1], w[:, 0]))
        s = w[order]
        start = np.concatenate([[True], (s[1:] != s[:-1]).any(1)])
        first = np.minimum.reduceat(ok[order], np.nonzero(start)[0])
        remap[ok[order]] = first[np.cumsum(start) - 1]
    return remap.astype(np.int32)


def _weld_apply_np(verts, faces):
    v, f = _host_mesh(verts, faces)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("weld: a face index lies outside [0, %d)" % v.shape[0])
    remap = weld_np(v)
    keep = remap == np.arange(v.shape[0])
    new_index = np.cumsum(keep) - 1
    return v[keep], new_index[remap[f]].astype(np.int32).reshape(-1, 3), remap


def components_np(n_verts, faces):
    """pnr_mesh_components' labels on the host, pure numpy: ``(vert_label (V,) int32, face_label (T,)
    int32, n_components)``.  Two vertices are connected when a face names both; a label is the lowest
    vertex index of the component; a vertex no face names is its own component.  Rounds of "every
    face lowers the labels of its vertices, and of their labels, to the face's minimum", each followed
    by pointer jumping to a fixed point, until nothing changes."""
    n_verts = int(n_verts)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= n_verts):
        raise ValueError("components: a face index lies outside [0, %d)" % n_verts)
    label = np.arange(n_verts, dtype=np.int64)
    while f.size:
        cur = label[f]
        low = cur.min(1)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, cur[:, k], low)
            np.minimum.at(new, f[:, k], low)
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, label):
            break
        label = new
    face_label = label[f[:, 0]] if f.size else np.zeros(0, np.int64)
    return label.astype(np.int32), face_label.astype(np.int32), int((label == np.arange(n_verts)).sum())


def _face_terms_np(verts, faces):
    """(area (T,), volume term (T,)) in fp64 from the fp32 vertices, in the header's operation order."""
    v, f = _host_mesh(verts, faces)
    v = v.astype(np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    nx, ny, nz = (u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                  u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0])
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    mx, my, mz = (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2],
                  b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
    return area, (a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz


def component_stats_np(verts, faces, vert_label, face_label):
    """ops.mesh_component_stats on the host: the same dict (numpy arrays).  The integer entries are
    those of the device; area and signed_volume are numpy's fp64 sums of the same per-face terms over
    each component's faces in ascending order (another summation order than the device's)."""
    vert_label, face_label = np.asarray(vert_label, np.int32), np.asarray(face_label, np.int32)
    labels = np.unique(vert_label)
    n_c = len(labels)
    vert_id, face_id = np.searchsorted(labels, vert_label), np.searchsorted(labels, face_label)
    cnt_v = np.bincount(vert_id, minlength=n_c).astype(np.int64)
    cnt_f = np.bincount(face_id, minlength=n_c).astype(np.int64)
    area, vol = np.zeros(n_c), np.zeros(n_c)
    if len(face_id):
        terms_a, terms_v = _face_terms_np(verts, faces)
        order = np.argsort(face_id, kind="stable")
        has = np.nonzero(cnt_f)[0]
        start = (np.cumsum(cnt_f) - cnt_f)[has]
        area[has] = np.add.reduceat(terms_a[order], start)
        vol[has] = np.add.reduceat(terms_v[order], start) / 6.0
    return {"labels": labels, "vert_id": vert_id.astype(np.int64), "face_id": face_id.astype(np.int64),
            "n_verts": cnt_v, "n_faces": cnt_f, "area": area, "signed_volume": vol}


def _np_poses(poses):
    p = poses.detach().cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses)
    p = np.ascontiguousarray(p, np.float32).astype(np.float64)
    if p.ndim != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError("poses must be (NV, 4, 4) or (NV, 3, 4) (got %s)" % (p.shape,))
    return p


def _pixel_dirs(width, height, fx, fy, cx, cy):
    """(X, -Y) of every pixel's direction (X, -Y, -1), (H W,) each, from the fp32 camera scalars."""
    fx, fy, cx, cy = (float(np.float32(t)) for t in (fx, fy, cx, cy))
    jj, ii = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    return ((ii - cx) / fx).reshape(-1), (-(jj - cy) / fy).reshape(-1)


def raycast_np(verts, faces, poses, width, height, focal, c=None, chunk=None):
    """pnr_mesh_raster's rule on the host (include/pnr_abi.h, "Mesh rendering"): ``(face (NV, H, W)
    int32, depth (NV, H, W) float64)`` by brute force over all pixels x faces in fp64 on the fp32
    inputs, ``chunk`` pixels at a time (default: about 2^21 pairs per step).  The same homogeneous hit
    rule (no two edge volumes of strictly opposite signs, not edge-on, depth > 0), the smallest
    camera-z depth wins and equal depths go to the lower face; faces with an index outside [0, V),
    a non-finite vertex or zero area, and views with a non-finite pose, contribute nothing."""
    from . import util

    v, f = _host_mesh(verts, faces)
    p = _np_poses(poses)
    width, height = int(width), int(height)
    fx, fy, cx, cy = util._focal_c(width, height, focal, c)
    X, Yn = _pixel_dirs(width, height, fx, fy, cx, cy)
    length = np.sqrt(X * X + Yn * Yn + 1.0)
    nv, hw = p.shape[0], width * height
    face = np.full((nv, hw), -1, np.int32)
    depth = np.zeros((nv, hw))
    ok = ((f >= 0) & (f < len(v))).all(1) if len(v) else np.zeros(len(f), bool)
    ids = np.nonzero(ok)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        tri = v.astype(np.float64)[f[ids]]                               # (T, 3, 3)
        area = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        good = np.isfinite(tri).all((1, 2)) & (area != 0).any(1) & np.isfinite(area).all(1)
    ids, tri = ids[good], tri[good]
    if len(ids) == 0:
        return face.reshape(nv, height, width), depth.reshape(nv, height, width)
    chunk = chunk or max(1, (1 << 21) // len(ids))
    for k in range(nv):
        if not np.isfinite(p[k, :3]).all():
            continue
        try:   # R^-1 (v - o), rows: the device takes the fp32 R for a rotation and uses R^T
            cam = (tri - p[k, :3, 3]) @ np.linalg.inv(p[k, :3, :3]).T
        except np.linalg.LinAlgError:
            continue
        a, b, cc = cam[:, 0], cam[:, 1], cam[:, 2]
        n_ab, n_bc, n_ca = np.cross(a, b), np.cross(b, cc), np.cross(cc, a)
        for i in range(0, hw, chunk):
            x, y = X[i:i + chunk, None], Yn[i:i + chunk, None]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                e_ab = x * n_ab[:, 0] + y * n_ab[:, 1] - n_ab[:, 2]
                e_bc = x * n_bc[:, 0] + y * n_bc[:, 1] - n_bc[:, 2]
                e_ca = x * n_ca[:, 0] + y * n_ca[:, 1] - n_ca[:, 2]
                pos = (e_ab > 0) | (e_bc > 0) | (e_ca > 0)
                neg = (e_ab < 0) | (e_bc < 0) | (e_ca < 0)
                det = e_ab + e_bc + e_ca
                s = -(e_bc * a[:, 2] + e_ca * b[:, 2] + e_ab * cc[:, 2]) / det
                hit = ~(pos & neg) & (det != 0) & (s > 0) & np.isfinite(s)
            s = np.where(hit, s, np.inf)
            best = s.argmin(1)                                          # the first minimum: the lowest face
            sb = s[np.arange(len(best)), best]
            got = np.isfinite(sb)
            face[k, i:i + chunk] = np.where(got, ids[best], -1)
            depth[k, i:i + chunk] = np.where(got, sb * length[i:i + chunk], 0.0)
    return face.reshape(nv, height, width), depth.reshape(nv, height, width)


def shade_np(verts, faces, poses, width, height, focal, face, depth, c=None, lights=(), weights=(),
             albedo=(0.8, 0.8, 0.8), ambient=0.2, background=(1.0, 1.0, 1.0)):
    """pnr_mesh_shade's formula in fp64 on the host: ``(rgb (NV, H, W, 3), normal (NV, H, W, 3))``
    float64 from the face and depth of a raster (include/pnr_abi.h, "Mesh rendering", Shading)."""
    from . import util

    v, f = _host_mesh(verts, faces)
    p = _np_poses(poses)
    width, height = int(width), int(height)
    fx, fy, cx, cy = util._focal_c(width, height, focal, c)
    X, Yn = _pixel_dirs(width, height, fx, fy, cx, cy)
    u = np.stack([X, Yn, -np.ones_like(X)], -1)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    face = np.asarray(face).reshape(p.shape[0], -1)
    depth = np.asarray(depth, np.float64).reshape(p.shape[0], -1)
    rgb = np.empty(face.shape + (3,))
    normal = np.zeros(face.shape + (3,))
    rgb[:] = np.asarray(background, np.float64)
    for k in range(p.shape[0]):
        m = face[k] >= 0
        if not m.any():
            continue
        tri = v.astype(np.float64)[f[face[k][m]]]
        d = u[m] @ p[k, :3, :3].T
        pt = p[k, :3, 3] + depth[k][m, None] * d
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where(((n * d).sum(1) > 0)[:, None], -n, n)
        lum = np.full(len(n), float(ambient))
        for L, w in zip(lights, weights):
            to = np.asarray(L, np.float64) - pt
            with np.errstate(invalid="ignore", divide="ignore"):
                cos = (n * to).sum(1) / np.linalg.norm(to, axis=1)
            lum += float(w) * np.where(cos > 0, cos, 0.0)
        rgb[k][m] = np.clip(np.asarray(albedo, np.float64) * lum[:, None], 0.0, 254.0 / 255.0)
        normal[k][m] = n
    shape = (p.shape[0], height, width, 3)
    return rgb.reshape(shape), normal.reshape(shape)
