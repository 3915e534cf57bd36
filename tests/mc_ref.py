"""numpy fp32 restatement of the isosurface semantics of include/pnr_abi.h ("Isosurface
extraction"): the reference the device extractor (csrc/mcubes.hip) is compared with, bit for bit.
Test infrastructure only.  It is driven by the case table it fetches through the ABI
(pnr_mc_case_table, a host call), and tests/test_mc_table.py shows on the CPU that table and
restatement are sound on their own (closed surfaces, Euler characteristics, second-order volume).

  inside     value > level (NaN: outside)
  vertex     on every grid edge whose ends differ, t = (level - a) / (b - a) from the lower-index
             end a to the higher b, NaN / negative -> 0, above 1 -> 1, coordinate = index + t, each
             operation one fp32 rounding
  ownership  grid point p = (x * ny + y) * nz + z owns its +x, +y, +z edges (axis 0, 1, 2)
  order      vertices by (owner point, axis); faces by (cell's minimum-corner point, table position)
  edge e     = 4 * axis + j: along `axis` from the cell corner whose two other coordinates (in
             increasing axis order) are (j & 1, j >> 1); corner k = (k & 1, (k >> 1) & 1, (k >> 2) & 1)
"""
import ctypes
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def case_table():
    """(256, 16) int8 from libpnr.so (loads without a GPU)."""
    from pnr import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.pnr_mc_case_table.restype = ctypes.c_int32
    lib.pnr_mc_case_table.argtypes = [ctypes.c_void_p]
    out = np.full((256, 16), 99, np.int8)
    rc = lib.pnr_mc_case_table(out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    out.setflags(write=False)
    return out


def corner_xyz(k):
    return (k & 1, (k >> 1) & 1, (k >> 2) & 1)


def edge_owner_offset(e):
    """(dx, dy, dz) of the owner corner of edge e, and its axis."""
    a, j = divmod(int(e), 4)
    others = [ax for ax in range(3) if ax != a]
    off = [0, 0, 0]
    off[others[0]], off[others[1]] = j & 1, j >> 1
    return tuple(off), a


def edge_ends(e):
    off, a = edge_owner_offset(e)
    hi = list(off)
    hi[a] = 1
    return off, tuple(hi)


def marching_cubes(grid, level, index_offset=(0, 0, 0)):
    """(verts (V, 3) float32, faces (T, 3) int32).  index_offset: `grid` is the block of a larger
    grid that starts at this index (the vertex indices then are those of the larger grid, if it
    has no crossing outside the block)."""
    g = np.ascontiguousarray(grid, dtype=np.float32)
    assert g.ndim == 3
    level = np.float32(level)
    nx, ny, nz = g.shape
    empty = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    if min(nx, ny, nz) < 2:
        return empty
    table = case_table()
    ntri = (table >= 0).sum(1) // 3
    with np.errstate(invalid="ignore"):
        inside = g > level
    n = nx * ny * nz
    # ---- vertices: (point, axis) in order; edge_map[point, axis] = vertex index or -1
    cross = np.zeros((nx, ny, nz, 3), bool)
    t = np.zeros((nx, ny, nz, 3), np.float32)
    sl = [slice(None)] * 3
    for a in range(3):
        lo, hi = list(sl), list(sl)
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross[lo + (a,)] = inside[lo] != inside[hi]
        with np.errstate(all="ignore"):
            ta = (level - g[lo]) / (g[hi] - g[lo])     # float32 throughout: one rounding each
        assert ta.dtype == np.float32
        ta = np.where(ta > 0, ta, np.float32(0))
        ta = np.where(ta < 1, ta, np.float32(1))
        t[lo + (a,)] = ta
    flat = cross.reshape(-1)
    edge_map = np.full(n * 3, -1, np.int64)
    where = np.nonzero(flat)[0]
    edge_map[where] = np.arange(where.size)
    p, a = where // 3, where % 3
    idx = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], 1)
    verts = (idx + np.asarray(index_offset, np.int64)).astype(np.float32)
    verts[np.arange(where.size), a] = verts[np.arange(where.size), a] + t.reshape(-1)[where]
    # ---- faces: (cell, table position) in order
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for k in range(8):
        dx, dy, dz = corner_xyz(k)
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << k
    ci, cj, ck = np.nonzero(ntri[case] > 0)
    cc = case[ci, cj, ck]
    cp = (ci * ny + cj) * nz + ck
    parts = []
    for q in range(5):
        m = ntri[cc] > q
        if not m.any():
            break
        tri = np.empty((int(m.sum()), 3), np.int64)
        for c in range(3):
            e = table[cc[m], 3 * q + c].astype(np.int64)
            ax, j = e // 4, e % 4
            u, v = j & 1, j >> 1
            dx = np.where(ax == 0, 0, u)
            dy = np.where(ax == 0, u, np.where(ax == 1, 0, v))
            dz = np.where(ax == 2, 0, v)
            owner = cp[m] + dx * (ny * nz) + dy * nz + dz
            tri[:, c] = edge_map[owner * 3 + ax]
        parts.append((cp[m], np.full(int(m.sum()), q), tri))
    if not parts:
        return verts, empty[1]
    cell = np.concatenate([x[0] for x in parts])
    pos = np.concatenate([x[1] for x in parts])
    tri = np.concatenate([x[2] for x in parts])
    order = np.lexsort((pos, cell))
    faces = tri[order]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32)


# ---- mesh measures shared by the CPU and GPU tests --------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces):
    """Every undirected edge in exactly two faces, once in each direction."""
    d = directed_edges(faces)
    if d.shape[0] == 0:
        return False
    key = d[:, 0] * (d.max() + 1) + d[:, 1]
    rev = d[:, 1] * (d.max() + 1) + d[:, 0]
    uk, cnt = np.unique(key, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(uk, np.unique(rev)))


def euler(verts, faces):
    d = directed_edges(faces)
    und = np.unique(np.sort(d, 1), axis=0)
    return int(len(verts)) - int(len(und)) + int(len(faces))


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---- analytic fixtures (index units) -----------------------------------------------------------
def _axes(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def sphere_grid(shape, center, radius):
    x, y, z = _axes(shape)
    c = center
    return (radius - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def torus_grid(shape, center, big_r, small_r):
    x, y, z = _axes(shape)
    c = center
    q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - big_r
    return (small_r - np.sqrt(q ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def two_spheres_grid(shape, c0, r0, c1, r1):
    return np.maximum(sphere_grid(shape, c0, r0), sphere_grid(shape, c1, r1))
