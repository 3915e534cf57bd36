"""Yardstick of the mesh-cleanup tests (a helper, not a conftest): the reference weld (np.unique over
the canonicalised rows, lowest index per class), the reference labelling (scipy's connected_components
over the face edges, relabelled to the lowest vertex index), fp64 per-component sums, and the meshes
the CPU and GPU tests share.  Semantics: include/pnr_abi.h, "Mesh cleanup"."""
import numpy as np

import mc_ref
import mesh_ref


# ---- references ------------------------------------------------------------------------------------
def weld(verts):
    """remap (V,) int64: the lowest index whose row equals row i as floats; NaN rows map to themselves."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    remap = np.arange(len(v), dtype=np.int64)
    ok = np.nonzero(~np.isnan(v).any(1))[0]
    if ok.size:
        canon = v[ok] + np.float32(0.0)   # -0.0 -> +0.0
        _, inv = np.unique(canon.view(np.uint32), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        low = np.full(inv.max() + 1, len(v), np.int64)
        np.minimum.at(low, inv, ok)
        remap[ok] = low[inv]
    return remap


def weld_mesh(verts, faces):
    """(verts', faces' int32, remap): the kept vertices in ascending order, the same T faces re-indexed."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    remap = weld(v)
    keep = remap == np.arange(len(v))
    new = np.cumsum(keep) - 1
    return v[keep], new[remap[np.asarray(faces, np.int64)]].astype(np.int32).reshape(-1, 3), remap


def components(n_verts, faces):
    """(vert_label (V,), face_label (T,), n_components) int64 with scipy's connected_components."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    rows = np.concatenate([f[:, 0], f[:, 1]])
    cols = np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_verts, n_verts))
    n, comp = connected_components(graph, directed=False)
    low = np.full(n, n_verts, np.int64)
    np.minimum.at(low, comp, np.arange(n_verts))
    label = low[comp]
    return label, (label[f[:, 0]] if len(f) else np.zeros(0, np.int64)), int(n)


def face_terms(verts, faces):
    """(area (T,), volume term (T,)) in fp64 from the fp32 vertices, the header's operation order."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    nx, ny, nz = (u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                  u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0])
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    mx, my, mz = (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2],
                  b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
    return area, (a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz


def stats(verts, faces, vert_label, face_label):
    """Per component in ascending label order: labels, n_verts, n_faces, area, signed_volume (numpy's
    fp64 sums), and abs_area / abs_volume = the sums of the terms' magnitudes (for the error bound)."""
    vert_label, face_label = np.asarray(vert_label, np.int64), np.asarray(face_label, np.int64)
    labels = np.unique(vert_label)
    fid = np.searchsorted(labels, face_label)
    ta, tv = face_terms(verts, faces) if len(face_label) else (np.zeros(0), np.zeros(0))
    out = {"labels": labels, "n_verts": np.bincount(np.searchsorted(labels, vert_label), minlength=len(labels)),
           "n_faces": np.bincount(fid, minlength=len(labels))}
    for key, terms, div in (("area", ta, 1.0), ("signed_volume", tv, 6.0)):
        out[key] = np.array([terms[fid == c].sum() / div for c in range(len(labels))])
        out["abs_" + key] = np.array([np.abs(terms[fid == c]).sum() / div for c in range(len(labels))])
    return out


def same_partition(a, b):
    """Whether two label vectors split their positions into the same classes."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.shape != b.shape:
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


# ---- meshes ------------------------------------------------------------------------------------------
def soup(verts, faces):
    """The STL soup of an indexed mesh: (verts (3 T, 3), faces = arange(3 T).reshape(T, 3))."""
    v = np.ascontiguousarray(np.asarray(verts, np.float32)[np.asarray(faces, np.int64)].reshape(-1, 3))
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def concat(*meshes):
    """Meshes one after another, indices shifted."""
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int32) + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def floater_scene():
    """(clean = icosphere(3), with_floater = clean + a 12-vertex icosphere of radius 0.02 at x = 2.5)."""
    clean = mesh_ref.icosphere(3)
    fv, ff = mesh_ref.icosphere(0, 0.02)
    return clean, concat(clean, (fv + np.array([2.5, 0, 0], np.float32), ff))


def three_spheres():
    """1,280 / 320 / 80 faces with radii 0.2 / 0.5 / 1.5: the face order is the reverse of the area
    order.  Components 0, 1, 2 in label order; areas about 0.5, 3.1, 26."""
    parts = [(mesh_ref.icosphere(3, 0.2), (0, 0, 0)), (mesh_ref.icosphere(2, 0.5), (3, 0, 0)),
             (mesh_ref.icosphere(1, 1.5), (0, 5, 0))]
    return concat(*[(v + np.array(c, np.float32), f) for (v, f), c in parts])


def permuted(verts, faces, seed):
    """Vertex ids and face rows shuffled by a fixed permutation: (verts', faces', perm) with
    verts'[perm[i]] = verts[i]."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(verts))
    v = np.empty_like(np.asarray(verts, np.float32))
    v[perm] = verts
    f = perm[np.asarray(faces, np.int64)].astype(np.int32)
    return v, np.ascontiguousarray(f[rng.permutation(len(f))]), perm


def strip(n_verts, order="reversed", seed=0):
    """A triangle strip over n_verts vertices (n_verts - 2 faces), vertex i at (i, i & 1, 0), its ids
    reversed or randomly permuted: one component, a chain as long as the mesh."""
    i = np.arange(n_verts)
    v = np.stack([i, i & 1, np.zeros_like(i)], 1).astype(np.float32)
    f = np.stack([i[:-2], i[1:-1], i[2:]], 1)
    perm = i[::-1].copy() if order == "reversed" else np.random.default_rng(seed).permutation(n_verts)
    out = np.empty_like(v)
    out[perm] = v
    return out, perm[f].astype(np.int32)


def fan(n_faces, hub):
    """n_faces triangles round one hub vertex (index `hub` of n_faces + 2 vertices)."""
    n = n_faces + 2
    rim = np.array([i for i in range(n) if i != hub])
    ang = np.linspace(0, 2 * np.pi, n - 1, endpoint=False)
    v = np.zeros((n, 3), np.float32)
    v[rim] = np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], 1)
    f = np.stack([np.full(n_faces, hub), rim[:-1], rim[1:]], 1)
    return v, f.astype(np.int32)


def islands(n_faces):
    """n_faces disjoint triangles (an unwelded soup of distinct points): n_faces components."""
    i = np.arange(3 * n_faces)
    v = np.stack([i, (i % 3 == 1), (i % 3 == 2)], 1).astype(np.float32)
    return v, i.reshape(-1, 3).astype(np.int32)


def blob_grid(res=32, n_spikes=20, seed=3):
    """A res^3 density grid with three blobs and n_spikes single-voxel spikes away from them, and its
    mc_ref mesh at level 0: (grid, verts, faces).  3 + n_spikes closed components."""
    g = np.maximum(mc_ref.two_spheres_grid((res,) * 3, (9.3, 9.7, 10.1), 5.2, (22.4, 21.6, 20.9), 4.3),
                   mc_ref.sphere_grid((res,) * 3, (8.6, 23.2, 22.7), 3.1))
    rng = np.random.default_rng(seed)
    placed = 0
    while placed < n_spikes:
        p = rng.integers(2, res - 2, 3)
        box = g[p[0] - 2:p[0] + 3, p[1] - 2:p[1] + 3, p[2] - 2:p[2] + 3]
        if (box > -1.0).any():   # too near a blob or another spike
            continue
        g[tuple(p)] = 0.7
        placed += 1
    v, f = mc_ref.marching_cubes(g, 0.0)
    return g, v, f


def shared_meshes():
    """name -> (verts, faces): the meshes both backends are compared on against the references."""
    (cv, cf), (fv, ff) = floater_scene()
    a = mesh_ref.icosphere(2)
    b = (mesh_ref.icosphere(1, 0.5)[0] + np.array([3, 0, 0], np.float32), mesh_ref.icosphere(1, 0.5)[1])
    two = permuted(*concat(a, b), seed=11)[:2]
    out = {"icosphere3": (cv, cf), "floater": (fv, ff), "floater_soup": soup(fv, ff), "two_shuffled": two,
           "strip_reversed": strip(4097, "reversed"), "strip_random": strip(4097, "random", seed=5),
           "fan": fan(2000, hub=777), "three_spheres": three_spheres(), "blob_grid": blob_grid()[1:],
           "one_face": (np.eye(3, dtype=np.float32), np.array([[2, 0, 1]], np.int32)),
           "no_faces": (np.arange(15, dtype=np.float32).reshape(5, 3), np.zeros((0, 3), np.int32))}
    out["blob_grid_soup"] = soup(*out["blob_grid"])
    return out
