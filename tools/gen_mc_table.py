#!/usr/bin/env python3
"""Generates pixel-nerf_amd/csrc/mc_table.h: the 256-case marching-cubes triangle table of
csrc/mcubes.hip (pnr_mc_case_table).

    python3 tools/gen_mc_table.py            writes the header
    python3 tools/gen_mc_table.py --check    fails if the committed header differs

Conventions (include/pnr_abi.h, "Isosurface extraction"):
  corner k of a cell     (dx, dy, dz) = (k & 1, (k >> 1) & 1, (k >> 2) & 1); case bit k = corner k inside
  edge e = 4 * axis + j  runs along `axis` from the corner whose two OTHER coordinates (in increasing
                         axis order) are (j & 1, j >> 1); its owner is that corner's grid point

The table is not typed in and not derived from the 15 base cases by symmetry (their complement
symmetry leaves holes).  Each case is built from its six faces:
  1. on every face the marching-squares segments of the face's four corner signs; a face whose two
     inside corners are diagonal is ambiguous and ALWAYS resolved the same way, by separating the
     inside corners (one segment around each).  The rule reads only that face's signs, so the two
     cells that share a face draw the same segments on it and closed surfaces come out closed;
  2. the segments are directed with the inside on a fixed side seen from outside the cell, so they
     chain into closed loops (every crossed edge has one segment in and one out);
  3. each loop is filled as a disk by a triangulation none of whose diagonals lies in a cell face
     (such a diagonal would be a face segment the neighbour does not have).
Triangles wind so that the right-hand normal points to the outside (lower values).  Largest case:
5 triangles.
"""
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "pixel-nerf_amd", "csrc", "mc_table.h")


def corner_xyz(k):
    return (k & 1, (k >> 1) & 1, (k >> 2) & 1)


def corner_index(p):
    return p[0] | (p[1] << 1) | (p[2] << 2)


def edge_ends(e):
    a, j = divmod(e, 4)
    others = [ax for ax in range(3) if ax != a]
    p = [0, 0, 0]
    p[others[0]], p[others[1]] = j & 1, j >> 1
    q = list(p)
    q[a] = 1
    return tuple(p), tuple(q)


EDGE_OF = {frozenset(edge_ends(e)): e for e in range(12)}


def edge_mid(e):
    p, q = edge_ends(e)
    return tuple((p[i] + q[i]) / 2.0 for i in range(3))


def faces():
    """[(axis, side, four corners in cyclic order)]"""
    out = []
    for a in range(3):
        others = [ax for ax in range(3) if ax != a]
        for s in (0, 1):
            cyc = []
            for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[a], p[others[0]], p[others[1]] = s, u, v
                cyc.append(tuple(p))
            out.append((a, s, cyc))
    return out


FACES = faces()


def sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def mean(ps):
    return tuple(sum(p[i] for p in ps) / float(len(ps)) for i in range(3))


def face_segments(case, face):
    """Directed marching-squares segments [(edge_from, edge_to)] of one face (inside on the left of
    the direction of travel when the face is seen from outside the cell)."""
    a, s, cyc = face
    inside = [bool(case >> corner_index(c) & 1) for c in cyc]
    fe = [EDGE_OF[frozenset((cyc[i], cyc[(i + 1) % 4]))] for i in range(4)]
    crossed = [i for i in range(4) if inside[i] != inside[(i + 1) % 4]]
    normal = tuple((1.0 if s else -1.0) if ax == a else 0.0 for ax in range(3))
    raw = []   # (edge, edge, vector from the segment towards its inside)
    if len(crossed) == 2:
        ins = [c for c, f in zip(cyc, inside) if f]
        outs = [c for c, f in zip(cyc, inside) if not f]
        raw.append((fe[crossed[0]], fe[crossed[1]], sub(mean(ins), mean(outs))))
    elif len(crossed) == 4:   # ambiguous: one segment around each inside corner
        for i in range(4):
            if inside[i]:
                e0, e1 = fe[(i - 1) % 4], fe[i]
                raw.append((e0, e1, sub(cyc[i], mean([edge_mid(e0), edge_mid(e1)]))))
    segs = []
    for e0, e1, to_inside in raw:
        d = sub(edge_mid(e1), edge_mid(e0))
        # outside normal x direction = left of the direction of travel, seen from outside
        if dot(cross(normal, d), to_inside) < 0:
            e0, e1 = e1, e0
        segs.append((e0, e1))
    return segs


def in_a_face(e0, e1):
    p0, q0 = edge_ends(e0)
    p1, q1 = edge_ends(e1)
    return any(p0[a] == q0[a] == p1[a] == q1[a] for a in range(3))


def triangulations(n):
    """Every triangulation of a convex n-gon 0..n-1 as a list of (i, j, k), i < j < k."""
    def rec(i, j):
        if j - i < 2:
            yield []
            return
        for k in range(i + 1, j):
            for left in rec(i, k):
                for right in rec(k, j):
                    yield left + right + [(i, k, j)]
    return rec(0, n - 1)


def fill(loop):
    n = len(loop)
    for tris in triangulations(n):
        ok = True
        for t in tris:
            for x, y in ((t[0], t[1]), (t[1], t[2]), (t[0], t[2])):
                if (y - x) % n in (1, n - 1):
                    continue   # a side of the loop: a face segment
                if in_a_face(loop[x], loop[y]):
                    ok = False
        if ok:
            return [tuple(loop[i] for i in t) for t in sorted(tris)]
    raise AssertionError("no admissible triangulation of loop %s" % (loop,))


def case_triangles(case):
    nxt = {}
    for f in FACES:
        for e0, e1 in face_segments(case, f):
            assert e0 not in nxt, (case, e0)
            nxt[e0] = e1
    assert sorted(nxt) == sorted(nxt.values())
    tris = []
    left = set(nxt)
    while left:
        start = min(left)
        loop, e = [], start
        while True:
            loop.append(e)
            left.discard(e)
            e = nxt[e]
            if e == start:
                break
        assert len(loop) >= 3, (case, loop)
        tris += fill(loop)
    return tris


def build():
    table = [case_triangles(c) for c in range(256)]
    # winding: corner 0 alone inside -> the normal points away from corner 0
    (t,) = table[1]
    m = [edge_mid(e) for e in t]
    if dot(cross(sub(m[1], m[0]), sub(m[2], m[0])), mean(m)) < 0:
        table = [[(a, c, b) for a, b, c in tris] for tris in table]
    assert max(len(t) for t in table) <= 5
    return table


def render(table):
    lines = [
        "// GENERATED by tools/gen_mc_table.py: do not edit.  The 256-case marching-cubes table of",
        "// mcubes.hip: per case up to 5 triangles as edge triples, -1 padded to 16 entries; edge",
        "// e = 4 * axis + j, corner k = (k & 1, (k >> 1) & 1, (k >> 2) & 1), case bit k = corner k",
        "// inside.  Included once per address space: define PNR_MC_TABLE_QUAL / PNR_MC_TABLE_NAME /",
        "// PNR_MC_NTRI_NAME before each include (no include guard on purpose).",
        "PNR_MC_TABLE_QUAL int8_t PNR_MC_TABLE_NAME[256][16] = {",
    ]
    for c, tris in enumerate(table):
        flat = [e for t in tris for e in t]
        flat += [-1] * (16 - len(flat))
        lines.append("    {%s},   // %d" % (", ".join("%2d" % v for v in flat), c))
    lines.append("};")
    lines.append("PNR_MC_TABLE_QUAL uint8_t PNR_MC_NTRI_NAME[256] = {")
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in table[r:r + 32]) + ",")
    lines.append("};")
    return "\n".join(lines) + "\n"


def main(argv):
    text = render(build())
    if "--check" in argv:
        if open(OUT).read() != text:
            print("mc_table.h is stale: run tools/gen_mc_table.py", file=sys.stderr)
            return 1
        return 0
    with open(OUT, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
