#!/usr/bin/env python
"""Derive the marching-cubes case table from the topology of the cube and write psnerf_amd/csrc/mc_table.h.

Conventions (those of the surface extractor the stage-1 model was published with, so that meshes agree cell face by cell face):
  corners  v0..v7 = (0,0,0) (1,0,0) (1,1,0) (0,1,0), then the same four with z + 1;
  edges    0..3 = v0v1 v1v2 v2v3 v3v0, 4..7 the same on the top face, 8..11 = v0v4 v1v5 v2v6 v3v7;
  case     bit m of the index is set iff value(v_m) <= iso value ("set" corners).

For every one of the 256 cases:
  1. the active edges are those whose two corners differ in their bit;
  2. a FACE WALK gives the boundary of the surface inside the cell: on every cube face with two active edges these are joined,
     on an ambiguous face (four active edges) every set corner is cut off separately;
  3. the segments close into loops of 3..7 vertices; every loop is oriented so that the normal of the surface points towards the
     set corners and is triangulated as a disc: the triangulations of the polygon are enumerated (apex of the closing edge first,
     then recursively both sides) and the first one is taken that uses no diagonal whose two cube edges lie in a common cube face
     (such a diagonal would lie IN that face and could overlap the neighbour cell's surface).

The result agrees with any other table built on the same face rule up to the choice of interior diagonals within a cell: same
vertices, same segment on every cell face (crack-free against any neighbour), same number of triangles.

    python tools/gen_mc_table.py            # rewrite the header
    python tools/gen_mc_table.py --check    # exit status 1 if the committed header differs
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'psnerf_amd', 'csrc', 'mc_table.h')

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
MAX_TRIS = 5


def _faces():
    """The six cube faces as (axis, side, corners in cyclic order, edges in the same order: edge i joins corner i and i + 1)."""
    faces = []
    for axis in range(3):
        for side in (0, 1):
            cs = [c for c in range(8) if CORNERS[c][axis] == side]
            # cyclic order: walk along cube edges
            order = [cs[0]]
            while len(order) < 4:
                for c in cs:
                    if c not in order and sum(abs(a - b) for a, b in zip(CORNERS[c], CORNERS[order[-1]])) == 1:
                        order.append(c)
                        break
            es = []
            for i in range(4):
                pair = {order[i], order[(i + 1) % 4]}
                es.append([e for e in range(12) if set(EDGES[e]) == pair][0])
            faces.append((axis, side, order, es))
    return faces


FACES = _faces()


def edges_share_face(a, b):
    return any(a in f[3] and b in f[3] for f in FACES)


def _mid(e):
    a, b = CORNERS[EDGES[e][0]], CORNERS[EDGES[e][1]]
    return tuple((x + y) / 2.0 for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def face_segments(case):
    """Directed segments (edge a -> edge b) of the face walk, directed so that the surface normal points to the set corners:
    with m the inward normal of the face and t the in-face direction from the segment towards the set corner(s) it cuts off,
    the surface lies to the left of a -> b seen along the normal, i.e. ((b - a) x m) . t > 0."""
    segs = []
    for axis, side, cs, es in FACES:
        bits = [(case >> c) & 1 for c in cs]
        active = [i for i in range(4) if bits[i] != bits[(i + 1) % 4]]
        if not active:
            continue
        m = [0.0, 0.0, 0.0]
        m[axis] = 1.0 if side == 0 else -1.0
        pairs = []
        if len(active) == 2:
            set_corners = [cs[i] for i in range(4) if bits[i]]
            pairs.append((es[active[0]], es[active[1]], set_corners))
        else:  # ambiguous: every set corner is cut off by the two face edges that meet in it
            for i in range(4):
                if bits[i]:
                    pairs.append((es[(i - 1) % 4], es[i], [cs[i]]))
        for a, b, set_corners in pairs:
            pa, pb = _mid(a), _mid(b)
            centre = tuple((x + y) / 2.0 for x, y in zip(pa, pb))
            sc = tuple(sum(CORNERS[c][k] for c in set_corners) / float(len(set_corners)) for k in range(3))
            t = _sub(sc, centre)
            if _dot(_cross(_sub(pb, pa), m), t) > 0:
                segs.append((a, b))
            else:
                segs.append((b, a))
    return segs


def loops(case):
    segs = face_segments(case)
    nxt = {}
    for a, b in segs:
        assert a not in nxt, 'edge %d leaves twice in case %d' % (a, case)
        nxt[a] = b
    assert sorted(nxt.keys()) == sorted(nxt.values())
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        out.append(loop)
    return out


def triangulations(poly):
    """All triangulations of the polygon (a list of vertex labels in cyclic order), each a list of triangles that keep the
    polygon's orientation; enumerated by the apex of the edge (last, first), lowest position first, then both sides."""
    k = len(poly)
    if k < 3:
        yield []
        return
    if k == 3:
        yield [tuple(poly)]
        return
    for m in range(1, k - 1):
        for left in triangulations(poly[:m + 1]):
            for right in triangulations(poly[m:]):
                yield left + [(poly[0], poly[m], poly[k - 1])] + right


def _diagonals(tris, loop):
    k = len(loop)
    boundary = set()
    for i in range(k):
        boundary.add(frozenset((loop[i], loop[(i + 1) % k])))
    out = set()
    for t in tris:
        for i in range(3):
            d = frozenset((t[i], t[(i + 1) % 3]))
            if d not in boundary:
                out.add(d)
    return out


def case_triangles(case):
    tris = []
    for loop in loops(case):
        assert 3 <= len(loop) <= 7
        for cand in triangulations(loop):
            if all(not edges_share_face(*tuple(d)) for d in _diagonals(cand, loop)):
                tris += cand
                break
        else:
            raise AssertionError('no admissible triangulation of loop %r in case %d' % (loop, case))
    assert len(tris) <= MAX_TRIS
    return tris


def table():
    return [case_triangles(c) for c in range(256)]


def render():
    tab = table()
    lines = ['// GENERATED by tools/gen_mc_table.py -- do not edit; `python tools/gen_mc_table.py --check` compares.',
             '// Marching-cubes case table derived from the cube topology (face walk; ambiguous faces cut off every corner whose',
             '// value is <= the iso value; loops triangulated as discs without in-face diagonals; normals towards those corners).',
             '// Corners v0..v7 = (0,0,0) (1,0,0) (1,1,0) (0,1,0) + the same with z+1; edges 0..3 = v0v1 v1v2 v2v3 v3v0, 4..7 on the',
             '// top face, 8..11 = v0v4 v1v5 v2v6 v3v7; bit m of the case index is set iff value(v_m) <= iso.',
             '#pragma once',
             '#ifndef PSN_MC_TABLE_ATTR  /* device code defines it as __device__ before including this file */',
             '#define PSN_MC_TABLE_ATTR',
             '#endif',
             '#define PSN_MC_MAX_TRIS %d' % MAX_TRIS,
             '// number of triangles per case',
             'PSN_MC_TABLE_ATTR static const unsigned char PSN_MC_NTRI[256] = {']
    for r in range(16):
        lines.append('    ' + ', '.join('%d' % len(tab[16 * r + c]) for c in range(16)) + ',')
    lines.append('};')
    lines.append('// cube edges of the triangle corners, %d per case, -1 terminated / padded' % (3 * MAX_TRIS + 1))
    lines.append('PSN_MC_TABLE_ATTR static const signed char PSN_MC_TRI[256][%d] = {' % (3 * MAX_TRIS + 1))
    for c in range(256):
        flat = [e for t in tab[c] for e in t]
        flat += [-1] * (3 * MAX_TRIS + 1 - len(flat))
        lines.append('    {' + ', '.join('%2d' % e for e in flat) + '},  // %3d' % c)
    lines.append('};')
    return '\n'.join(lines) + '\n'


def main():
    text = render()
    if '--check' in sys.argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print('mc_table.h is %s' % ('up to date' if same else 'OUT OF DATE'))
        sys.exit(0 if same else 1)
    with open(HEADER, 'w') as f:
        f.write(text)
    print('wrote', HEADER)


if __name__ == '__main__':
    main()
