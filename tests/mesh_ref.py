"""Yardstick of the mesh-metric tests (a helper, not a conftest): the numpy fp64 restatement of
pnr_mesh_sample's rule (include/pnr_abi.h, "Mesh metrics") built on oracle/philox.py, a brute-force
fp64 nearest neighbour, the score formulas of Occupancy Networks' eval_pointcloud, and meshes."""
import subprocess

import numpy as np

from oracle import philox

RNG_MESH = 4   # PNR_RNG_MESH
U = 2.0 ** -24


def icosphere(subdivisions, radius=1.0):
    """(verts (V, 3) float32, faces (T, 3) int32) of an icosahedron subdivided `subdivisions` times,
    every vertex on the sphere of `radius`, outward winding.  T = 20 * 4^subdivisions."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def face_geometry(verts, faces):
    """(areas (T,), cross products (T, 3), their lengths (T,)) in fp64 from the fp32 vertices, in the
    operation order the header fixes."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    cr = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                   u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)
    ln = np.sqrt(cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1] + cr[:, 2] * cr[:, 2])
    return 0.5 * ln, cr, ln


def sample(verts, faces, n, seed):
    """The restatement: a dict with tri (n,), points (n, 3) fp64 (the exact-arithmetic combination of
    the fp32 vertices with the fp32 barycentrics, evaluated in fp64), normals (n, 3) fp64, total,
    and `near_boundary`, the number of samples whose target lies within T * 2^-52 * total of a CDF
    boundary (where another fixed summation order may pick the neighbouring face)."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    area, cr, ln = face_geometry(verts, faces)
    cdf = np.cumsum(area)
    total = float(cdf[-1])
    u = philox.stream(seed, 0, RNG_MESH, n, 3)
    assert u.dtype == np.float32 and u.shape == (n, 3)
    target = u[:, 0].astype(np.float64) * total
    tri = np.minimum(np.searchsorted(cdf, target, side="right"), len(cdf) - 1)
    # the CDF is sorted: the boundaries nearest to a target are the two that bracket it
    slack = len(cdf) * 2.0 ** -52 * total
    below = np.where(tri > 0, cdf[np.maximum(tri - 1, 0)], -np.inf)
    near = int((np.minimum(cdf[tri] - target, target - below) <= slack).sum())
    u1, u2 = u[:, 1].copy(), u[:, 2].copy()
    fold = (u1 + u2) > np.float32(1.0)          # the fp32 sum
    u1[fold], u2[fold] = np.float32(1.0) - u1[fold], np.float32(1.0) - u2[fold]
    a, b, c = v[f[tri, 0]], v[f[tri, 1]], v[f[tri, 2]]
    points = a + u1.astype(np.float64)[:, None] * (b - a) + u2.astype(np.float64)[:, None] * (c - a)
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = cr[tri] / ln[tri][:, None]
    return {"tri": tri, "points": points, "normals": normals, "total": total, "near_boundary": near, "area": area}


def sqdist(a, b_rows):
    """Row-wise fp64 squared distance of fp32 points."""
    d = np.asarray(a, np.float32).astype(np.float64) - np.asarray(b_rows, np.float32).astype(np.float64)
    return (d * d).sum(-1)


def nearest(a, b, chunk=512):
    """Brute force in fp64 on the fp32 inputs: (min_j D(i, j), the lowest j that attains it)."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    dmin = np.empty(len(a))
    idx = np.empty(len(a), np.int64)
    for i in range(0, len(a), chunk):
        d = a[i:i + chunk, None, :] - b[None, :, :]
        dd = (d * d).sum(-1)
        idx[i:i + chunk] = dd.argmin(1)
        dmin[i:i + chunk] = dd.min(1)
    return dmin, idx


def scores(pa, na, pb, nb, tau):
    """The ten scores in fp64 from two fp32 clouds and their normals, and the two distance fields."""
    d2_ab, i_ab = nearest(pa, pb)
    d2_ba, i_ba = nearest(pb, pa)
    d_ab, d_ba = np.sqrt(d2_ab), np.sqrt(d2_ba)
    na, nb = np.asarray(na, np.float64), np.asarray(nb, np.float64)
    acc, comp = d_ab.mean(), d_ba.mean()
    prec, rec = (d_ab < tau).mean(), (d_ba < tau).mean()
    nacc = np.abs((na * nb[i_ab]).sum(-1)).mean()
    ncomp = np.abs((nb * na[i_ba]).sum(-1)).mean()
    out = {"accuracy": acc, "completeness": comp, "chamfer_l1": 0.5 * (acc + comp),
           "chamfer_l2": 0.5 * (d2_ab.mean() + d2_ba.mean()), "precision": prec, "recall": rec,
           "fscore": 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0, "normals_accuracy": nacc,
           "normals_completeness": ncomp, "normal_consistency": 0.5 * (nacc + ncomp)}
    return {k: float(x) for k, x in out.items()}, d_ab, d_ba


def to_index_units(verts, res):
    """World coordinates in [-1, 1]^3 -> the index units scripts/eval.py writes on a res^3 grid."""
    return ((np.asarray(verts, np.float64) + 1.0) * (res - 1) / 2.0).astype(np.float32)


def write_eval_tree(root, res, objects):
    """A scratch tree as scripts/eval.py leaves it and its ground truth: objects = {name: (radius of
    the predicted sphere in world units, radius of the ground-truth sphere or None for no file)}.
    Returns (output dir, ground-truth dir)."""
    import os

    from pnr import mesh

    out, gt = os.path.join(root, "eval"), os.path.join(root, "gt")
    os.makedirs(gt)
    for name, (r_pred, r_gt) in objects.items():
        os.makedirs(os.path.join(out, name))
        v, f = icosphere(3, r_pred)
        mesh.write_stl(os.path.join(out, name, name + "_mesh.stl"), to_index_units(v, res), f)
        if r_gt is not None:
            v, f = icosphere(3, r_gt)
            mesh.write_stl(os.path.join(gt, name + ".stl"), v + np.float32(0.25), f)   # off-centre: normalised away
    return out, gt


# for the eval_mesh.py tests: run the script, read a metrics file as rows of words or as {name: value}
def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def _lines(path):
    with open(path) as fh:
        return [ln.split() for ln in fh.read().split("\n")[:-1]]


def _read(path):
    with open(path) as fh:
        return {k: float(x) for k, x in (ln.split() for ln in fh)}


def sphere_slack(subdivisions, radius, n_samples):
    """(sagitta of the icosphere's largest face, expected nearest-sample spacing): the face's
    circumradius is at most its longest edge over sqrt(3) (the faces are acute), a face inscribed in
    the sphere of radius R with circumradius c lies R - sqrt(R^2 - c^2) below it at its centre; n
    uniform samples on an area A lie about sqrt(A / n) apart."""
    v, f = icosphere(subdivisions, radius)
    v = v.astype(np.float64)
    edge = max(np.linalg.norm(v[f[:, i]] - v[f[:, (i + 1) % 3]], axis=1).max() for i in range(3))
    sag = radius - np.sqrt(radius ** 2 - edge ** 2 / 3.0)
    return float(sag), float(np.sqrt(face_geometry(v, f)[0].sum() / n_samples))
