"""The marching-cubes case table of csrc/mcubes.hip, fetched through the ABI (pnr_mc_case_table, a
host call: no GPU), and the numpy restatement tests/mc_ref.py that the device tests compare with.

Table, all 256 cases: (a) triangle vertices sit on sign-changing edges; (b) on each of the six
faces the triangle edges lying in the face are exactly the marching-squares segments of the
face's four corner signs, the ambiguous face always separating its inside corners, so adjacent
cells agree and closed surfaces come out closed; (c) every other triangle edge is used twice,
once per direction; (d) winding: normals point away from the inside; (e) cases 0 and 255 are
empty.  mc_ref: closed surfaces of Euler characteristic 2 / 0 / 4 on a sphere / torus / two
spheres, and second-order convergence of the sphere's volume.
"""
import collections
import math
import os

import numpy as np

import mc_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tris(row):
    vals = [int(v) for v in row]
    n = sum(v >= 0 for v in vals)
    assert n % 3 == 0 and all(v >= 0 for v in vals[:n]) and all(v == -1 for v in vals[n:]), vals
    assert all(0 <= v < 12 for v in vals[:n])
    return [tuple(vals[i:i + 3]) for i in range(0, n, 3)]


def _inside(case, corner):
    return bool(case >> (corner[0] | corner[1] << 1 | corner[2] << 2) & 1)


def _faces_of_cell():
    out = []
    for a in range(3):
        o = [ax for ax in range(3) if ax != a]
        for s in (0, 1):
            cyc = []
            for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[a], p[o[0]], p[o[1]] = s, u, v
                cyc.append(tuple(p))
            out.append((a, s, cyc))
    return out


EDGE_OF = {frozenset(mc_ref.edge_ends(e)): e for e in range(12)}


def _squares_segments(case, cyc):
    """Undirected marching-squares segments of one face; ambiguous: one around each inside corner."""
    ins = [_inside(case, c) for c in cyc]
    fe = [EDGE_OF[frozenset((cyc[i], cyc[(i + 1) % 4]))] for i in range(4)]
    crossed = [i for i in range(4) if ins[i] != ins[(i + 1) % 4]]
    if len(crossed) == 2:
        return [frozenset((fe[crossed[0]], fe[crossed[1]]))]
    if len(crossed) == 4:
        return [frozenset((fe[(i - 1) % 4], fe[i])) for i in range(4) if ins[i]]
    assert not crossed
    return []


def test_table_shape_and_empty_cases():
    t = mc_ref.case_table()
    assert t.shape == (256, 16) and t.dtype == np.int8
    assert (t[0] == -1).all() and (t[255] == -1).all()                       # (e)
    assert all(1 <= len(_tris(t[c])) <= 5 for c in range(1, 255))


def test_triangle_vertices_lie_on_sign_changing_edges():                      # (a)
    t = mc_ref.case_table()
    for c in range(256):
        used = {e for tri in _tris(t[c]) for e in tri}
        crossing = {e for e in range(12)
                    if _inside(c, mc_ref.edge_ends(e)[0]) != _inside(c, mc_ref.edge_ends(e)[1])}
        assert used == crossing, (c, used, crossing)     # every crossing edge carries the surface, no other
        for tri in _tris(t[c]):
            assert len(set(tri)) == 3, (c, tri)


def test_faces_carry_exactly_the_marching_squares_segments():                 # (b) and (c)
    t = mc_ref.case_table()
    faces = _faces_of_cell()
    for c in range(256):
        directed = collections.Counter()
        for a, b, d in _tris(t[c]):
            directed.update([(a, b), (b, d), (d, a)])
        on_face = collections.Counter()
        for (e0, e1), n in directed.items():
            ends = mc_ref.edge_ends(e0) + mc_ref.edge_ends(e1)
            shared = [(ax, s) for ax in range(3) for s in (0, 1) if all(p[ax] == s for p in ends)]
            if shared:
                assert len(shared) == 1
                on_face[(shared[0], frozenset((e0, e1)))] += n
            else:   # (c): an interior edge, once in each direction
                assert n == 1 and directed[(e1, e0)] == 1, (c, e0, e1)
        want = collections.Counter()
        for ax, s, cyc in faces:
            for seg in _squares_segments(c, cyc):
                want[((ax, s), seg)] += 1
        assert on_face == want, (c, on_face, want)


def test_winding_points_away_from_the_inside():                               # (d)
    t = mc_ref.case_table()
    mid = lambda e: np.mean(np.array(mc_ref.edge_ends(e), np.float64), 0)  # noqa: E731
    for k in range(8):
        (tri,) = _tris(t[1 << k])
        p = [mid(e) for e in tri]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        assert np.dot(n, np.mean(p, 0) - np.array(mc_ref.corner_xyz(k), np.float64)) > 0, k
        # the complement: one corner outside, the normal points towards it
        tris = _tris(t[255 ^ (1 << k)])
        assert len(tris) == 1
        p = [mid(e) for e in tris[0]]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        assert np.dot(n, np.array(mc_ref.corner_xyz(k), np.float64) - np.mean(p, 0)) > 0, k


def test_committed_header_is_what_the_generator_emits():
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(REPO, "tools", "gen_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    table = gen.build()
    assert open(gen.OUT).read() == gen.render(table), "csrc/mc_table.h is stale: run tools/gen_mc_table.py"
    got = mc_ref.case_table()
    for c in range(256):
        assert _tris(got[c]) == table[c], c


# ---- tests/mc_ref.py by itself -----------------------------------------------------------------
def _sphere_volume_error(n, center, radius):
    """|enclosed volume - 4/3 pi R^3| in units of the coarse grid, on an n-times refined grid."""
    shape = tuple(24 * n - (n - 1) for _ in range(3))
    g = mc_ref.sphere_grid(shape, [c * n for c in center], radius * n)
    v, f = mc_ref.marching_cubes(g, 0.0)
    assert mc_ref.is_closed_oriented(f) and mc_ref.euler(v, f) == 2
    return abs(mc_ref.signed_volume(v, f) / n ** 3 - 4.0 / 3.0 * math.pi * radius ** 3), mc_ref.signed_volume(v, f)


def test_ref_sphere_is_closed_and_its_volume_converges_at_second_order():
    center, radius = (11.3, 11.7, 12.1), 8.3
    e1, vol = _sphere_volume_error(1, center, radius)
    e2, _ = _sphere_volume_error(2, center, radius)
    print("sphere R = %.1f h: volume error %.4f (h), %.4f (h / 2), ratio %.2f; relative %.2e, %.2e" % (
        radius, e1, e2, e1 / e2, e1 / (4 / 3 * math.pi * radius ** 3), e2 / (4 / 3 * math.pi * radius ** 3)))
    assert vol > 0
    assert e1 / e2 >= 3.0, (e1, e2)


def test_ref_torus_and_two_spheres_topology():
    g = mc_ref.torus_grid((26, 27, 12), (12.4, 13.1, 5.6), 7.2, 3.1)
    v, f = mc_ref.marching_cubes(g, 0.0)
    assert mc_ref.is_closed_oriented(f) and mc_ref.euler(v, f) == 0 and mc_ref.signed_volume(v, f) > 0
    g = mc_ref.two_spheres_grid((30, 16, 15), (7.2, 7.9, 7.4), 5.3, (21.6, 8.1, 7.3), 5.8)
    v, f = mc_ref.marching_cubes(g, 0.0)
    assert mc_ref.is_closed_oriented(f) and mc_ref.euler(v, f) == 4 and mc_ref.signed_volume(v, f) > 0


def test_ref_degenerate_inputs():
    g = mc_ref.sphere_grid((9, 9, 9), (4, 4, 4), 3.2)
    for lvl in (100.0, -100.0):
        v, f = mc_ref.marching_cubes(g, lvl)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = mc_ref.marching_cubes(g[:, :1, :], 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    # a vertex exactly at a grid point (value == level is outside): t = 0 or 1, finite
    g2 = np.zeros((3, 3, 3), np.float32)
    g2[1, 1, 1] = 1.0
    v, f = mc_ref.marching_cubes(g2, 0.0)
    assert len(v) == 6 and len(f) == 8 and mc_ref.is_closed_oriented(f) and np.isfinite(v).all()
