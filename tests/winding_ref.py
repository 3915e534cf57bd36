"""Yardstick of the mesh-containment tests (a helper, not a conftest): the generalized winding number
of include/pnr_abi.h, "Mesh containment", restated in numpy twice.

  winding64  the formula in fp64 on the fp32 inputs: the reference of every comparison
  winding32  the header's rule operation by operation in fp32, fmas where the header puts them (an
             fp32 fma is the fp64 product-sum of fp32 values rounded to fp32: the product is exact in
             fp64, and the second rounding moves the result only on a tie), the sum in fp64: the host
             emulation of the device arithmetic.  It differs from the device in atan2f alone.

A face with an index outside [0, V) contributes 0 in both, as on the device."""
import numpy as np

F32, F64 = np.float32, np.float64


def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _dot32(ax, ay, az, bx, by, bz):
    return _fma(az, bz, _fma(ay, by, ax * bx))


def _omega64(ax, ay, az, bx, by, bz, cx, cy, cz):
    la = np.sqrt(ax * ax + ay * ay + az * az)
    lb = np.sqrt(bx * bx + by * by + bz * bz)
    lc = np.sqrt(cx * cx + cy * cy + cz * cz)
    num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
    den = (la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la
           + (cx * ax + cy * ay + cz * az) * lb)
    return 2.0 * np.arctan2(num, den)                     # arctan2(0, 0) = 0: a query on a vertex


def _omega32(ax, ay, az, bx, by, bz, cx, cy, cz):
    la = np.sqrt(_dot32(ax, ay, az, ax, ay, az))
    lb = np.sqrt(_dot32(bx, by, bz, bx, by, bz))
    lc = np.sqrt(_dot32(cx, cy, cz, cx, cy, cz))
    ab, bc, ca = _dot32(ax, ay, az, bx, by, bz), _dot32(bx, by, bz, cx, cy, cz), _dot32(cx, cy, cz, ax, ay, az)
    nx, ny, nz = by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx      # unfused
    num = _dot32(ax, ay, az, nx, ny, nz)
    den = _fma(ca, lb, _fma(bc, la, _fma(ab, lc, (la * lb) * lc)))
    omega = F32(2.0) * np.arctan2(num, den)
    assert omega.dtype == F32
    return omega


def _pairs(v, f, p, dtype, chunk):
    v = np.asarray(v, np.float32).reshape(-1, 3).astype(dtype)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    p = np.asarray(p, np.float32).reshape(-1, 3).astype(dtype)
    f = f[((f >= 0) & (f < len(v))).all(1)]
    out = np.zeros(len(p), np.float64)
    if len(f) == 0:
        return out
    tri = [v[f[:, k], c][None, :] for k in range(3) for c in range(3)]
    chunk = chunk or max(1, (1 << 21) // len(f))
    omega = _omega64 if dtype is F64 else _omega32
    with np.errstate(invalid="ignore"):
        for i in range(0, len(p), chunk):
            q = [p[i:i + chunk, c, None] for c in range(3)]
            out[i:i + chunk] = omega(*(tri[3 * k + c] - q[c] for k in range(3) for c in range(3))).astype(F64).sum(-1)
    return out / (4.0 * np.pi)


def winding64(v, f, p, chunk=None):
    """(n,) float64: the winding number of the mesh (v fp32, f) at the fp32 points p, in fp64."""
    return _pairs(v, f, p, np.float64, chunk)


def winding32(v, f, p, chunk=None):
    """(n,) float64: the device's per-pair fp32 arithmetic (numpy's atan2f for the device's), the sum
    over the faces in fp64."""
    return _pairs(v, f, p, np.float32, chunk)


def near_sphere(center, radius, n, eps, rng):
    """n fp32 points within eps * radius of the sphere an icosphere is inscribed in: uniform
    directions, radii uniform in radius * [1 - eps, 1 + eps]."""
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(center, np.float64) + d * (radius * (1.0 + rng.uniform(-eps, eps, (n, 1))))).astype(np.float32)


def near_faces(verts, faces, n, eps, rng):
    """n fp32 points within eps of the mesh's faces themselves: a random point of a random face, moved
    along the face's normal by a uniform offset in [-eps, eps].  Some land within eps of an edge."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    t = rng.integers(0, len(f), n)
    a, b, c = v[f[t, 0]], v[f[t, 1]], v[f[t, 2]]
    u = rng.uniform(0, 1, (n, 2))
    u[u.sum(1) > 1] = 1 - u[u.sum(1) > 1]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return (a + u[:, :1] * (b - a) + u[:, 1:] * (c - a) + rng.uniform(-eps, eps, (n, 1)) * nrm).astype(np.float32)
