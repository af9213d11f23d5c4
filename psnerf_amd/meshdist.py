"""Mesh evaluation: surface sampling, point-to-mesh distance and the reference's Chamfer distance (chamfer_dist.py:19-35 at the top
of the reference tree; stage2/utils/metrics.py:79-113 is the same function with its raw outputs, and the one-sided
``get_surface_dist``).  The reference does this with trimesh.sample.sample_surface + trimesh.proximity.closest_point (trimesh and
rtree); neither is needed here.

Two implementations of one definition, as in stage1/extracting.py:
  * CPU inputs -> the vectorised numpy functions below (``host_*``), float64; they are the definition, and what the device path is
    tested against.
  * device tensors (or ``device='cuda'``) -> csrc/meshdist.hip through ``MeshIndex``: a uniform grid of triangle lists over the
    mesh's bounding box (psn_tri_grid_count -> torch.cumsum -> psn_tri_grid_fill), then psn_closest_point, which walks shells of
    cells around each query's home cell and stops by an exact bound.  Meshes, samples and distances stay on the device; the uniforms
    of the sampler are drawn on the host from the caller's ``np.random.RandomState`` in the host path's order and uploaded, so both
    paths consume the same stream.

Definition.  distance(p, mesh) = min over ALL triangles of the Euclidean distance from p to the triangle as the closed convex
hull of its three corners (Ericson, Real-Time Collision Detection, 5.1.5: the Voronoi-region test, which needs no division by the
area).  Ties on the distance go to the lowest triangle index.
Stated difference from the reference: trimesh yields NaN for degenerate (zero-area) triangles and the reference zeroes those
distances (chamfer_dist.py:27-28); here such a triangle is the segment or point it degenerates to and takes part with its true
distance, so no NaN arises and nothing is zeroed.
Sampling is trimesh.sample.sample_surface as documented: faces with probability proportional to their area, a uniform point in
the face from two uniforms with the reflection u + v > 1 -> (1 - u, 1 - v).  The distribution is the contract; the order of the
draws (all face picks, then all (u, v) pairs) is this module's own.

Ray casting (the reference has none: every depth, normal and shadow map of its comes from marching the occupancy network) follows
the same pattern: ``host_ray_cast`` is the definition, csrc/meshray.hip through ``MeshIndex.ray_cast`` the device path over the same
grid.  Definition.  A ray o + t d hits a triangle by the watertight test of Woop, Benthin and Wald (JCGT 2013), without back-face
culling and with t_min <= t <= t_max; the result per ray is the minimum of (t, triangle index) in lexicographic order over ALL
triangles; a miss is t = inf, triangle -1, NaN barycentrics.  With ``any_hit`` only the boolean is defined.
Stated differences from what a plain Moeller-Trumbore caster returns: a triangle with det == 0 (zero area, or seen edge-on) is never
hit; a ray with a NaN (or infinite) component or a zero direction misses.

The inside test (the reference has none either) likewise: ``host_crossings`` is the definition, csrc/meshinside.hip through
``MeshIndex.crossings`` / ``contains`` the device path.  Definition.  The line through a point along a coordinate axis crosses a
triangle by the same edge functions without the shear, with an edge function that is exactly 0 decided by simulation of simplicity,
so that a line through a shared edge or a vertex crosses exactly one of the triangles around it; per point the triangles of the
WHOLE mesh crossed above it, below it and at it are counted, and inside = the parity of those above.
"""
import numpy as np
import torch

from .meshcore import Phase, device_mesh, face_areas, host_mesh, mesh_parts, on_device, to_numpy
from .meshcore import load_mesh   # noqa: F401 (the evaluation tools and tests read meshes through this module)

_PAIRS_PER_CHUNK = 1 << 20   # host path: point-triangle pairs evaluated at a time (some forty float64 temporaries of that size)


# ------------------------------------------------------------------------------------------------ host path: the definition
def _dot(ax, ay, az, bx, by, bz):
    return ax * bx + ay * by + az * bz


def _segment(p, a, b):
    """The point of segment [a, b] closest to p, per component (a zero-length segment is the point a)."""
    e = [b[i] - a[i] for i in range(3)]
    num = _dot(e[0], e[1], e[2], p[0] - a[0], p[1] - a[1], p[2] - a[2])
    den = _dot(e[0], e[1], e[2], e[0], e[1], e[2])
    s = np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)
    s = np.where(s < 0.0, 0.0, np.where(s > 1.0, 1.0, s))
    return [a[i] + s * e[i] for i in range(3)]


def _dist2(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return dx * dx + dy * dy + dz * dz


def _closest_on_triangles(p, a, b, c):
    """Closest point of triangles (a, b, c) to points p; every argument a list of three broadcastable float64 arrays (x, y, z).
    Ericson 5.1.5, operation for operation as csrc/meshdist.hip:md_closest -> list of three arrays."""
    with np.errstate(all='ignore'):
        ab = [b[i] - a[i] for i in range(3)]
        ac = [c[i] - a[i] for i in range(3)]
        ap = [p[i] - a[i] for i in range(3)]
        d1, d2 = _dot(*ab, *ap), _dot(*ac, *ap)
        bp = [p[i] - b[i] for i in range(3)]
        d3, d4 = _dot(*ab, *bp), _dot(*ac, *bp)
        cp = [p[i] - c[i] for i in range(3)]
        d5, d6 = _dot(*ab, *cp), _dot(*ac, *cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        r_a = (d1 <= 0.0) & (d2 <= 0.0)
        r_b = (d3 >= 0.0) & (d4 <= d3)
        r_c = (d6 >= 0.0) & (d5 <= d6)
        # (an edge of zero length -- a repeated corner -- is no edge region: its test would pass trivially and return the corner)
        r_ab = (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0) & (d1 - d3 > 0.0)
        r_ac = (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0) & (d2 - d6 > 0.0)
        r_bc = (va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0) & (e43 + e56 > 0.0)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        s = va + vb + vc
        v, w = vb / s, vc / s
        r_in = (s > 0.0) & (v >= 0.0) & (w >= 0.0) & (v + w <= 1.0)
        # the fall-back for what rounding lets through every test: the best of the three edges
        q1, q2, q3 = _segment(p, a, b), _segment(p, a, c), _segment(p, b, c)
        e1, e2, e3 = _dist2(p, q1), _dist2(p, q2), _dist2(p, q3)
        use2 = e2 < e1
        best = np.where(use2, e2, e1)
        use3 = e3 < best
        out = []
        for i in range(3):
            fb = np.where(use3, q3[i], np.where(use2, q2[i], q1[i]))
            out.append(np.select([r_a, r_b, r_c, r_ab, r_ac, r_bc, r_in],
                                 [a[i], b[i], c[i], a[i] + v_ab * ab[i], a[i] + w_ac * ac[i],
                                  b[i] + w_bc * (c[i] - b[i]), a[i] + ab[i] * v + ac[i] * w], fb))
        return out


def host_point_triangle(vertices, faces, points, triangle_id):
    """Closest point and distance from points [Q, 3] to the triangles triangle_id [Q] (one triangle per point) ->
    (closest float64 [Q, 3], distance float64 [Q])."""
    v, f, _ = host_mesh(vertices, faces)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = f[np.asarray(triangle_id, dtype=np.int64)]
    p = [pts[:, i] for i in range(3)]
    q = _closest_on_triangles(p, *[[v[t[:, k], i] for i in range(3)] for k in range(3)])
    return np.stack(q, axis=1), np.sqrt(_dist2(p, q))


def host_closest_point(vertices, faces, points):
    """The return triple of trimesh.proximity.closest_point(mesh, points): (closest float64 [Q, 3], distance float64 [Q],
    triangle_id int64 [Q]) by brute force over all triangles, in chunks of queries so that memory stays bounded.  Ties on the
    distance go to the lowest triangle index.  Unlike trimesh, zero-area triangles take part with their true (segment / point)
    distance and no NaN arises (see the module docstring)."""
    v, f, _ = host_mesh(vertices, faces)
    if f.shape[0] == 0:
        raise ValueError('host_closest_point: the mesh has no faces')
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    n_q = pts.shape[0]
    tri_id = np.zeros(n_q, dtype=np.int64)
    corners = [[v[f[:, k], i][None, :] for i in range(3)] for k in range(3)]
    step = max(1, _PAIRS_PER_CHUNK // f.shape[0])
    for q0 in range(0, n_q, step):
        p = [pts[q0:q0 + step, i][:, None] for i in range(3)]
        d2 = _dist2(p, _closest_on_triangles(p, *corners))
        tri_id[q0:q0 + step] = np.argmin(d2, axis=1)            # (the first minimum: the lowest index)
    closest, dist = host_point_triangle(v, f, pts, tri_id)
    return closest, dist, tri_id


def _ray_frames(origins, directions):
    """Per ray the frame of the watertight test: (valid [Q], k int64 [Q, 3] = (kx, ky, kz), o [Q, 3] = the origin in that order,
    S [Q, 3] = (Sx, Sy, Sz)).  kz = the axis of the largest |d| (the first on a tie), kx, ky the next two cyclically, swapped when
    d[kz] < 0.  Rays with a non-finite component or a zero direction are not valid (their frame is a placeholder)."""
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError('rays: origins %s and directions %s differ in shape' % (o.shape, d.shape))
    valid = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0.0).any(axis=1)
    d = np.where(valid[:, None], d, np.array([0.0, 0.0, 1.0]))
    o = np.where(valid[:, None], o, 0.0)
    kz = np.argmax(np.abs(d), axis=1)            # (the first maximum)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    rows = np.arange(len(d))
    swap = d[rows, kz] < 0.0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    k = np.stack([kx, ky, kz], axis=1)
    dk = d[rows, kz]
    S = np.stack([d[rows, kx] / dk, d[rows, ky] / dk, 1.0 / dk], axis=1)
    return valid, k, np.take_along_axis(o, k, axis=1), S


def _ray_triangles(o, S, a, b, c):
    """The watertight ray-triangle test of Woop, Benthin and Wald (JCGT 2013), operation for operation as csrc/meshray.hip:mr_test.
    o, S: lists of three broadcastable arrays, the origin and the shear constants in the ray's (kx, ky, kz) order; a, b, c: the
    corners in the same order -> (accepted, t, U, V, W, det); t_min / t_max are the caller's."""
    with np.errstate(all='ignore'):
        Akz, Bkz, Ckz = a[2] - o[2], b[2] - o[2], c[2] - o[2]
        Ax, Ay = (a[0] - o[0]) - S[0] * Akz, (a[1] - o[1]) - S[1] * Akz
        Bx, By = (b[0] - o[0]) - S[0] * Bkz, (b[1] - o[1]) - S[1] * Bkz
        Cx, Cy = (c[0] - o[0]) - S[0] * Ckz, (c[1] - o[1]) - S[1] * Ckz
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        same = ((U >= 0.0) & (V >= 0.0) & (W >= 0.0)) | ((U <= 0.0) & (V <= 0.0) & (W <= 0.0))
        det = U + V + W
        ok = same & (det != 0.0)
        Az, Bz, Cz = S[2] * Akz, S[2] * Bkz, S[2] * Ckz
        t = (U * Az + V * Bz + W * Cz) / det
        return ok, t, U, V, W, det


def host_ray_triangle(vertices, faces, origins, directions, triangle_id):
    """The watertight test of rays [Q] against the triangles triangle_id [Q] (one triangle per ray), without a window on t ->
    (t float64 [Q], barycentrics float64 [Q, 3] = (U, V, W) / det, accepted bool [Q]).  Where the test does not accept (or the id is
    negative) t is inf and the barycentrics are NaN."""
    v, f, _ = host_mesh(vertices, faces)
    valid, k, o, S = _ray_frames(origins, directions)
    tid = np.asarray(triangle_id, dtype=np.int64).reshape(-1)
    valid = valid & (tid >= 0)
    corners = v[f[np.where(tid >= 0, tid, 0)]]                   # [Q, 3 corners, 3 axes]
    a, b, c = (np.take_along_axis(corners[:, i, :], k, axis=1) for i in range(3))
    ok, t, U, V, W, det = _ray_triangles([o[:, i] for i in range(3)], [S[:, i] for i in range(3)], [a[:, i] for i in range(3)],
                                         [b[:, i] for i in range(3)], [c[:, i] for i in range(3)])
    ok = ok & valid
    with np.errstate(all='ignore'):
        bary = np.where(ok[:, None], np.stack([U / det, V / det, W / det], axis=1), np.nan)
    return np.where(ok, t, np.inf), bary, ok


def host_ray_cast(vertices, faces, origins, directions, t_min=0.0, t_max=np.inf, any_hit=False):
    """Rays origins + t directions [Q, 3] against the mesh by brute force over all triangles, in chunks of rays so that memory stays
    bounded -> (t float64 [Q], triangle_id int64 [Q], barycentrics float64 [Q, 3], hit bool [Q]): the first accepted hit with
    t_min <= t <= t_max, ties on t to the lowest triangle index; a miss is (inf, -1, NaN, False).  ``any_hit``: only ``hit`` is
    computed, the other three hold the values of a miss.  See the module docstring for the definition."""
    v, f, _ = host_mesh(vertices, faces)
    if f.shape[0] == 0:
        raise ValueError('host_ray_cast: the mesh has no faces')
    if not t_min <= t_max:
        raise ValueError('host_ray_cast: t_min=%r > t_max=%r' % (t_min, t_max))
    valid, k, o, S = _ray_frames(origins, directions)
    n_q = len(valid)
    tri = np.full(n_q, -1, dtype=np.int64)
    hit = np.zeros(n_q, dtype=bool)
    step = max(1, _PAIRS_PER_CHUNK // f.shape[0])
    code = k[:, 0] * 3 + k[:, 2]                                 # one value per (kx, ky, kz): rays of one frame share the corner order
    for frame in np.unique(code[valid]):
        rows = np.nonzero(valid & (code == frame))[0]
        kk = k[rows[0]]
        corners = [[v[f[:, j], kk[i]][None, :] for i in range(3)] for j in range(3)]
        for q0 in range(0, len(rows), step):
            r = rows[q0:q0 + step]
            ok, t, _, _, _, _ = _ray_triangles([o[r, i][:, None] for i in range(3)], [S[r, i][:, None] for i in range(3)], *corners)
            with np.errstate(invalid='ignore'):
                ok &= (t >= t_min) & (t <= t_max)
            hit[r] = ok.any(axis=1)
            tri[r] = np.where(hit[r], np.argmin(np.where(ok, t, np.inf), axis=1), -1)     # (the first minimum: the lowest index)
    if any_hit:
        tri[:] = -1
    t, bary, _ = host_ray_triangle(v, f, origins, directions, tri)
    return t, tri, bary, hit


def _side(e, Px, Py, Qx, Qy):
    """The side of the directed edge (P, Q) on which the line lies, by simulation of simplicity (the line moved by (+d, +d^2) in
    (kx, ky)): sign(e), or where e == 0 sign(Qy - Py), or where that is 0 sign(Px - Qx) -> int8; antisymmetric in (P, Q).  A NaN e
    gives 0."""
    one, zero = np.int8(1), np.int8(0)
    sign = lambda pos, neg: np.where(pos, one, np.where(neg, -one, zero))
    tie = sign(Qy > Py, Qy < Py)
    return np.where(e == 0.0, np.where(tie != 0, tie, sign(Px > Qx, Px < Qx)), sign(e > 0.0, e < 0.0))


def _line_triangles(p, a, b, c):
    """The line through p along kz against triangles (a, b, c), operation for operation as csrc/meshinside.hip:mi_count.  p, a, b, c:
    lists of three broadcastable arrays in (kx, ky, kz) order -> (accepted, z): the watertight ray test with S = (0, 0, 1), written
    without the shear, and with ties on an edge function decided by ``_side``."""
    with np.errstate(all='ignore'):
        Ax, Ay, Az = a[0] - p[0], a[1] - p[1], a[2] - p[2]
        Bx, By, Bz = b[0] - p[0], b[1] - p[1], b[2] - p[2]
        Cx, Cy, Cz = c[0] - p[0], c[1] - p[1], c[2] - p[2]
        box = ((np.minimum(np.minimum(Ax, Bx), Cx) <= 0.0) & (np.maximum(np.maximum(Ax, Bx), Cx) >= 0.0) &
               (np.minimum(np.minimum(Ay, By), Cy) <= 0.0) & (np.maximum(np.maximum(Ay, By), Cy) >= 0.0))
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        sU, sV, sW = _side(U, Bx, By, Cx, Cy), _side(V, Cx, Cy, Ax, Ay), _side(W, Ax, Ay, Bx, By)
        det = U + V + W
        ok = box & (sU != 0) & (sU == sV) & (sU == sW) & (det != 0.0)
        z = (U * Az + V * Bz + W * Cz) / det
        return ok & np.isfinite(z), z


def host_crossings(vertices, faces, points, axis=2):
    """How often the line through each of points [Q, 3] along ``axis`` crosses the mesh, by brute force over all triangles in chunks
    of points -> (above int32 [Q], below int32 [Q], on int32 [Q]): the triangles crossed above the point (z > 0), below it and exactly
    at it.  inside = above & 1; (above + below + on) & 1 = the line does not see a closed surface.

    Definition.  kz = axis, kx = (axis + 1) % 3, ky = (axis + 2) % 3.  Per triangle the corners are translated by -p, U, V, W are the
    edge functions of ``_ray_triangles`` and each one's side is ``_side``: a point exactly on an edge or a vertex of the projected
    mesh belongs to exactly one of two triangles on opposite sides of that edge, so a parity over a closed surface is exact also for
    lines through vertices and edges.  A triangle counts when the line lies in the closed bounding box of its projection (exact
    comparisons; implied by the sides in exact arithmetic, and there for slivers whose U, V, W are all rounding noise: their signs
    can agree for a point anywhere on the slivers' line), the three sides are equal and non-zero and det = U + V + W != 0, with
    z = (U Az + V Bz + W Cz) / det; a non-finite z counts nowhere.  Zero-area and edge-on triangles are never counted; a point with a
    non-finite coordinate gets three zeros."""
    v, f, _ = host_mesh(vertices, faces)
    if f.shape[0] == 0:
        raise ValueError('host_crossings: the mesh has no faces')
    if axis not in (0, 1, 2):
        raise ValueError('host_crossings: axis=%r (0, 1 or 2)' % (axis,))
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    k = [(axis + 1) % 3, (axis + 2) % 3, axis]
    counts = np.zeros((3, pts.shape[0]), dtype=np.int32)
    rows = np.nonzero(np.isfinite(pts).all(axis=1))[0]
    corners = [[v[f[:, j], k[i]][None, :] for i in range(3)] for j in range(3)]
    step = max(1, _PAIRS_PER_CHUNK // f.shape[0])
    for q0 in range(0, len(rows), step):
        r = rows[q0:q0 + step]
        ok, z = _line_triangles([pts[r, k[i]][:, None] for i in range(3)], *corners)
        counts[0, r] = (ok & (z > 0.0)).sum(axis=1)
        counts[1, r] = (ok & (z < 0.0)).sum(axis=1)
        counts[2, r] = (ok & (z == 0.0)).sum(axis=1)
    return counts[0], counts[1], counts[2]


def host_face_areas(vertices, faces):
    v, f, _ = host_mesh(vertices, faces)
    return face_areas(v, f)


def _draw(rng, count):
    """The uniforms of one sample_surface call, in this module's order: ``count`` face picks, then ``count`` (u, v) pairs."""
    rng = np.random if rng is None else rng
    pick = rng.random_sample(count)
    uv = rng.random_sample((count, 2))
    return pick, uv


def host_sample_surface(vertices, faces, count, rng=None, return_cumulative=False):
    """trimesh.sample.sample_surface(mesh, count) -> (points float64 [count, 3], face_index int64 [count]): faces drawn with
    probability proportional to their area, a uniform point per draw.  ``rng``: an np.random.RandomState (default: the global
    np.random, as the reference)."""
    v, f, _ = host_mesh(vertices, faces)
    if f.shape[0] == 0:
        raise ValueError('host_sample_surface: the mesh has no faces')
    pick, uv = _draw(rng, int(count))
    area_cum = np.cumsum(host_face_areas(v, f))
    face_index = np.minimum(np.searchsorted(area_cum, pick * area_cum[-1]), f.shape[0] - 1).astype(np.int64)
    u, w = uv[:, 0], uv[:, 1]
    flip = u + w > 1.0
    u, w = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - w, w)
    a, b, c = v[f[face_index, 0]], v[f[face_index, 1]], v[f[face_index, 2]]
    points = a + u[:, None] * (b - a) + w[:, None] * (c - a)
    return (points, face_index, area_cum) if return_cumulative else (points, face_index)


def host_tri_grid(vertices, faces, lo, hi, cell, n, max_span):
    """The triangle grid (PsnTriGrid with its lists) that csrc/meshdist.hip builds, as plain float64 numpy: the definition of the
    index every device query walks, operation for operation as csrc/trigrid.h (md_cell, md_range) -> dict(c0 int64 [F, 3],
    c1 int64 [F, 3]: each triangle's first and last cell per axis; span int64 [F]: the cells of that range; over int64: the ids of
    the oversize triangles (span > max_span), ascending; cell_count int64 [cells]; cell_start int64 [cells + 1]: the exclusive scan
    of the counts with the total appended; list int64 [n_entries]: per cell the ids of the triangles whose range holds it and that
    are not oversize, ascending within the cell).  The linear index of cell (x, y, z) is (x n[1] + y) n[2] + z.  ``hi`` is part of
    the descriptor and of no formula here: a coordinate beyond lo + n cell clamps into the last cell."""
    v, f, _ = host_mesh(vertices, faces)
    n = [int(k) for k in n]
    inv = 1.0 / float(cell)
    corners = v[f]                                               # [F, 3 corners, 3 axes]
    c0 = np.zeros((f.shape[0], 3), dtype=np.int64)
    c1 = np.zeros((f.shape[0], 3), dtype=np.int64)
    for a in range(3):
        for out, x in ((c0, corners[:, :, a].min(axis=1)), (c1, corners[:, :, a].max(axis=1))):
            with np.errstate(invalid='ignore'):
                t = np.floor((x - float(lo[a])) * inv)
                t = np.where(t >= 0.0, t, 0.0)                   # (a t that is not >= 0, a NaN among them, goes to 0)
                out[:, a] = np.where(t > float(n[a] - 1), float(n[a] - 1), t).astype(np.int64)
    extent = c1 - c0 + 1
    span = extent[:, 0] * extent[:, 1] * extent[:, 2]
    is_over = span > int(max_span)
    cells = n[0] * n[1] * n[2]
    entries = []                                                 # per listed triangle: its cells, then its id as often
    for t in np.nonzero(~is_over)[0]:
        x, y, z = np.meshgrid(*[np.arange(c0[t, a], c1[t, a] + 1) for a in range(3)], indexing='ij')
        entries.append(np.stack([((x * n[1] + y) * n[2] + z).ravel(), np.full(x.size, t, dtype=np.int64)]))
    entries = np.concatenate(entries, axis=1) if entries else np.zeros((2, 0), dtype=np.int64)
    order = np.lexsort((entries[1], entries[0]))                 # by cell, then by id
    cell_count = np.bincount(entries[0], minlength=cells).astype(np.int64)
    cell_start = np.concatenate([[0], np.cumsum(cell_count)]).astype(np.int64)
    return dict(c0=c0, c1=c1, span=span, over=np.nonzero(is_over)[0].astype(np.int64), cell_count=cell_count, cell_start=cell_start,
                list=entries[1][order])


# ------------------------------------------------------------------------------------------------ device path
MAX_SPAN = 256      # a triangle whose bounding box overlaps more cells than this goes to the oversize list
CELLS_PER_AXIS = 192   # at most 192^3 = 7.1 M cells: a 28 MB table of list starts


def grid_shape(lo, hi, mean_edge, cell=None):
    """The grid MeshIndex lays over the bounding box [lo, hi] of a mesh with the mean triangle edge ``mean_edge`` -> (cell, n): cell =
    max(mean edge, largest extent / CELLS_PER_AXIS) unless the caller gives one, 1 where that is not positive (every vertex in one
    point); n[a] = ceil(extent[a] / cell) within 1 .. CELLS_PER_AXIS.  A given cell so small that an axis would need more than
    CELLS_PER_AXIS cells leaves a truncated grid, lo[a] + n[a] cell < hi[a]: the last cell of that axis then holds everything
    beyond it (``grid_truncated``)."""
    extent = [hi[i] - lo[i] for i in range(3)]
    if cell is None:
        cell = max(mean_edge if np.isfinite(mean_edge) else 0.0, max(extent) / CELLS_PER_AXIS)
    if not cell > 0.0:
        cell = 1.0   # every vertex in one point
    n = [int(min(CELLS_PER_AXIS, max(1, np.ceil(extent[i] / cell)))) for i in range(3)]
    return cell, n


def grid_truncated(lo, hi, cell, n):
    """Does the grid stop short of the bounding box on some axis (lo + n cell < hi, in the grid's own rounding)?"""
    return any(lo[i] + n[i] * cell < hi[i] for i in range(3))


class MeshIndex(object):
    """A mesh on the device with its triangle grid: ``MeshIndex(vertices, faces).closest_point(points)``; one index serves any
    number of queries.  vertices float64 [V, 3] / faces int64 [F, 3]: device tensors, or numpy arrays / CPU tensors that are moved
    to ``device`` once.  Cell edge = max(mean triangle edge, largest box extent / CELLS_PER_AXIS); triangles that span more than
    MAX_SPAN cells (a few long slivers of a scan) are kept in a short list that every query tests directly, so they neither fail
    nor inflate the cell lists; ``cell`` and ``max_span`` override the two.  Two host reads while building: (bounding box, mean edge,
    index range) and the list totals.  ``index`` is the built index as the hip.* queries take it."""

    def __init__(self, vertices, faces, device=None, name='mesh', profile=False, cell=None, max_span=MAX_SPAN):
        from . import hip
        self.vertices, self.faces, _ = device_mesh(vertices, faces, None, device)
        device = self.vertices.device
        if self.faces.shape[0] == 0 or self.vertices.shape[0] == 0:
            raise ValueError('%s is empty (%d vertices, %d faces)' % (name, self.vertices.shape[0], self.faces.shape[0]))
        v, f = self.vertices, self.faces
        a, b, c = v[f[:, 0].clamp(0, v.shape[0] - 1)], v[f[:, 1].clamp(0, v.shape[0] - 1)], v[f[:, 2].clamp(0, v.shape[0] - 1)]
        edge = ((b - a).norm(dim=1) + (c - b).norm(dim=1) + (a - c).norm(dim=1)).mean() / 3.0
        head = torch.cat([v.min(dim=0).values, v.max(dim=0).values, edge.reshape(1), f.min().to(torch.float64).reshape(1),
                          f.max().to(torch.float64).reshape(1)]).tolist()
        lo, hi, mean_edge, f_min, f_max = head[0:3], head[3:6], head[6], int(head[7]), int(head[8])
        if f_min < 0 or f_max >= v.shape[0]:
            raise ValueError('%s: a face refers to vertex %d of %d' % (name, f_max if f_max >= v.shape[0] else f_min, v.shape[0]))
        if not all(np.isfinite(lo + hi)):
            raise ValueError('%s: a vertex coordinate is not finite' % name)
        cell, n = grid_shape(lo, hi, mean_edge, cell)
        self.lo, self.hi, self.cell, self.n = lo, hi, cell, n
        self.grid = hip.tri_grid(lo, hi, cell, n, max_span)
        self.build_events = [] if profile else None   # (phase, start event, end event) of the build (tools/bench_chamfer.py)
        counts = torch.zeros(2, dtype=torch.int64, device=device)
        with self._phase('count'):
            cell_count, over_list = hip.tri_grid_count(self.grid, v, f, counts[0:1])
        with self._phase('scan'):
            incl = torch.cumsum(cell_count, dim=0, dtype=torch.int64)
            counts[1] = incl[-1]
        n_over, n_entries = (int(x) for x in counts.tolist())
        if n_entries >= 2 ** 31:
            raise RuntimeError('%s: %d cell-list entries do not fit 32-bit positions' % (name, n_entries))
        with self._phase('scan'):
            self.cell_start = torch.zeros(cell_count.numel() + 1, dtype=torch.int32, device=device)
            self.cell_start[1:] = incl
            cursor = self.cell_start[:-1].clone()
        with self._phase('fill'):   # (no entries: every triangle is oversize, and the list is never read)
            self.list = hip.tri_grid_fill(self.grid, v, f, cursor, n_entries) if n_entries else torch.zeros(1, dtype=torch.int32, device=device)
        self.over_list, self.n_over, self.n_entries = over_list[:n_over].clone(), n_over, n_entries
        self.index = hip.mesh_index(self.grid, v, f, self.cell_start, self.list, self.over_list, n_over)

    def _phase(self, name):
        return Phase(self.build_events, name)

    @property
    def index_bytes(self):
        return 4 * (self.cell_start.numel() + self.list.numel() + self.over_list.numel())

    def home_order(self, points, axes=(0, 1, 2)):
        """The permutation that sorts the points by their (clamped) home cell: plumbing that keeps a wave's lanes in neighbouring
        cells.  It only orders the work; the kernel forms the home cell itself.  ``axes``: the grid axes from the slowest to the
        fastest digit of the sort key (the default is the cells' own linear index)."""
        lo = torch.tensor(self.lo, dtype=torch.float64, device=points.device)
        top = torch.tensor(self.n, dtype=torch.float64, device=points.device) - 1.0
        c = torch.nan_to_num(torch.floor((points - lo) / self.cell), nan=0.0)
        c = torch.minimum(torch.clamp(c, min=0.0), top).to(torch.int64)
        key = (c[:, axes[0]] * self.n[axes[1]] + c[:, axes[1]]) * self.n[axes[2]] + c[:, axes[2]]
        return torch.sort(key).indices

    def closest_point(self, points, n_tests=None):
        """points float64 [Q, 3] on the index's device -> (closest [Q, 3], distance [Q], triangle_id int64 [Q]), device tensors.
        n_tests: an int64 [1] device tensor to which the number of point-triangle tests is added."""
        from . import hip
        if not (torch.is_tensor(points) and points.is_cuda):
            raise RuntimeError('MeshIndex.closest_point: points must be a device tensor (host arrays: host_closest_point)')
        points = points.to(torch.float64).reshape(-1, 3).contiguous()
        order = self.home_order(points) if points.shape[0] > 64 else None   # (one wave: nothing to order)
        return hip.closest_point(self.index, points, order=order, n_tests=n_tests)

    def entry_order(self, origins, directions, t_min=0.0):
        """The permutation that sorts the rays by the cell in which they enter the bounding box (the cell of the origin at t_min when
        that lies inside; rays that miss the box go by their clamped origin): what home_order is for points.  It only orders the
        work; the kernel clips and walks the ray itself."""
        lo = torch.tensor(self.lo, dtype=torch.float64, device=origins.device)
        hi = torch.tensor(self.hi, dtype=torch.float64, device=origins.device)
        inv = 1.0 / directions
        t0, t1 = (lo - origins) * inv, (hi - origins) * inv
        t_in = torch.nan_to_num(torch.minimum(t0, t1), nan=-float('inf')).max(dim=1).values
        t_in = torch.nan_to_num(torch.clamp(t_in, min=t_min), nan=0.0, posinf=0.0, neginf=0.0)
        return self.home_order(origins + t_in[:, None] * directions)

    def ray_cast(self, origins, directions, t_min=0.0, t_max=float('inf'), any_hit=False, n_tests=None, sort=True):
        """origins / directions float64 [Q, 3] on the index's device -> (t [Q], triangle_id int64 [Q], barycentrics [Q, 3], hit bool [Q]),
        device tensors: host_ray_cast on the device.  n_tests: an int64 [1] device tensor to which the number of ray-triangle tests is
        added.  sort=False: the rays are worked on in the order given (a caller that hands over coherent bundles, meshrender's
        8 x 8 pixel tiles)."""
        from . import hip
        if not (torch.is_tensor(origins) and origins.is_cuda and torch.is_tensor(directions) and directions.is_cuda):
            raise RuntimeError('MeshIndex.ray_cast: origins and directions must be device tensors (host arrays: host_ray_cast)')
        origins = origins.to(torch.float64).reshape(-1, 3).contiguous()
        directions = directions.to(torch.float64).reshape(-1, 3).contiguous()
        order = self.entry_order(origins, directions, t_min) if sort and origins.shape[0] > 64 else None   # (one wave: nothing to order)
        t, tri, bary, hit = hip.ray_cast(self.index, origins, directions, t_min, t_max, order=order, any_hit=any_hit, n_tests=n_tests)
        return t, tri, bary, hit.bool()

    def crossings(self, points, axis=2, below=True, n_tests=None, sort=True):
        """points float64 [Q, 3] on the index's device -> (above, below, on) int32 [Q], device tensors: host_crossings on the device
        (csrc/meshinside.hip).  below=False: only the part of the line above each point is walked; ``below`` is then None, ``above``
        and ``on`` are the same integers.  The points are worked on sorted by column, then by cell along ``axis`` (sort=False: in
        the order given); that only orders the work.  n_tests: an int64 [1] device tensor to which the number of line-triangle tests
        is added."""
        from . import hip
        if not (torch.is_tensor(points) and points.is_cuda):
            raise RuntimeError('MeshIndex.crossings: points must be a device tensor (host arrays: host_crossings)')
        if axis not in (0, 1, 2):
            raise ValueError('MeshIndex.crossings: axis=%r (0, 1 or 2)' % (axis,))
        points = points.to(torch.float64).reshape(-1, 3).contiguous()
        axes = ((axis + 1) % 3, (axis + 2) % 3, axis)
        order = self.home_order(points, axes) if sort and points.shape[0] > 64 else None   # (one wave: nothing to order)
        return hip.mesh_crossings(self.index, points, axis=axis, order=order, want_below=below, n_tests=n_tests)

    def contains(self, points, axis=2, vote=False):
        """Is each of points [Q, 3] inside the mesh -> bool [Q]: the parity of the crossings above the point along ``axis``.  Exact
        for a closed surface, also for points whose line runs through vertices and edges (see host_crossings); for a point ON the
        surface the answer depends on the axis.  vote=True: the majority of the three axes (``axis`` is not used), for scans with
        holes, where a line through a hole has the wrong parity."""
        return _contains(self, points, axis, vote)

    def occlusion(self, points, normals, table, local=True, bias=0.0, t_max=float('inf'), bits=False, n_tests=None, out=None):
        """points / normals float64 [R, 3] on the index's device, table float64 [K, 3] (a device tensor, or a numpy array that is
        uploaded) -> (hits int32 [R], visible int32 [R], ao [R], bent [R, 3], words int32 [R, ceil(K / 32)] or None), device tensors:
        meshocclude.host_occlusion_rows on the device (csrc/meshocclude.hip).  The rows are worked on in the order given: consecutive
        rows should be neighbours on the surface, as the rows of an atlas are.  n_tests: an int64 [1] device tensor to which the
        number of ray-triangle tests is added."""
        from . import hip
        if not (torch.is_tensor(points) and points.is_cuda and torch.is_tensor(normals) and normals.is_cuda):
            raise RuntimeError('MeshIndex.occlusion: points and normals must be device tensors (host arrays: meshocclude.host_occlusion_rows)')
        points = points.to(torch.float64).reshape(-1, 3).contiguous()
        normals = normals.to(torch.float64).reshape(-1, 3).contiguous()
        if not torch.is_tensor(table):
            table = torch.from_numpy(np.ascontiguousarray(np.asarray(table, dtype=np.float64)))
        table = table.to(device=points.device, dtype=torch.float64).contiguous()
        return hip.occlusion_rows(self.index, points, normals, table, local=local, bias=bias, t_max=t_max, bits=bits, n_tests=n_tests, out=out)

    def project_rows(self, points, normals, images, views, hw=None, masks=None, bias=0.0, cos_min=0.0, weight='cosine', frame='raw',
                     bits=False, n_tests=None, out=None):
        """points / normals float64 [R, 3] on the index's device; images uint8 or float32 [V, H, W, C] (or None with ``hw`` = (H, W):
        visibility only); views float64 [V, 16] (hull._views); masks [V, H, W] or None -- device tensors, or numpy arrays that are
        uploaded -> meshproject.Projection of device tensors: meshproject.host_project_rows on the device (csrc/meshproject.hip).
        The rows are worked on in the order given: consecutive rows should be neighbours on the surface, as the rows of an atlas
        and the vertices of an extracted mesh are.  n_tests: an int64 [1] device tensor to which the ray-triangle tests are added."""
        from . import hip
        from .meshproject import Projection, check_modes
        if not (torch.is_tensor(points) and points.is_cuda and torch.is_tensor(normals) and normals.is_cuda):
            raise RuntimeError('MeshIndex.project_rows: points and normals must be device tensors (host arrays: meshproject.host_project_rows)')
        uniform, camera_normal = check_modes(weight, frame, 'MeshIndex.project_rows')
        points = points.to(torch.float64).reshape(-1, 3).contiguous()
        normals = normals.to(torch.float64).reshape(-1, 3).contiguous()
        dev = points.device
        place = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.array(x))).to(dev).contiguous()   # (a copy: read-only arrays)
        views = place(views).to(torch.float64)
        if images is not None:
            images = place(images)
        if masks is not None:
            masks = place(masks)
            masks = masks.view(torch.uint8) if masks.dtype == torch.bool else (masks if masks.dtype == torch.uint8 else (masks != 0).view(torch.uint8))
        return Projection(*hip.project_rows(self.index, points, normals, views, images, hw=hw, masks=masks, bias=bias, cos_min=cos_min,
                                            uniform=uniform, camera_normal=camera_normal, bits=bits, n_tests=n_tests, out=out))

    def face_areas_cumulative(self):
        return torch.cumsum(face_areas(self.vertices, self.faces), dim=0)

    def sample_surface(self, count, rng=None, return_cumulative=False):
        """host_sample_surface on the device: the uniforms are drawn on the host from ``rng`` in the host path's order and uploaded
        (3 x count doubles); areas, their cumulative sum, the search and the barycentric step run on the device."""
        pick, uv = _draw(rng, int(count))
        dev = self.vertices.device
        pick, uv = torch.from_numpy(pick).to(dev), torch.from_numpy(uv).to(dev)
        area_cum = self.face_areas_cumulative()
        face_index = torch.clamp(torch.searchsorted(area_cum, pick * area_cum[-1]), max=self.faces.shape[0] - 1)
        u, w = uv[:, 0], uv[:, 1]
        flip = u + w > 1.0
        u, w = torch.where(flip, 1.0 - u, u), torch.where(flip, 1.0 - w, w)
        t = self.faces[face_index]
        a, b, c = self.vertices[t[:, 0]], self.vertices[t[:, 1]], self.vertices[t[:, 2]]
        points = a + u[:, None] * (b - a) + w[:, None] * (c - a)
        return (points, face_index, area_cum) if return_cumulative else (points, face_index)


class _HostMesh(object):
    """The host twin of MeshIndex (same methods), so that the Chamfer functions below and meshrender are written once."""

    def __init__(self, vertices, faces, name='mesh'):
        self.vertices, self.faces, _ = host_mesh(vertices, faces)
        if self.faces.shape[0] == 0 or self.vertices.shape[0] == 0:
            raise ValueError('%s is empty (%d vertices, %d faces)' % (name, self.vertices.shape[0], self.faces.shape[0]))

    def sample_surface(self, count, rng=None):
        return host_sample_surface(self.vertices, self.faces, count, rng)

    def closest_point(self, points):
        return host_closest_point(self.vertices, self.faces, points)

    def ray_cast(self, origins, directions, t_min=0.0, t_max=np.inf, any_hit=False, n_tests=None):
        return host_ray_cast(self.vertices, self.faces, to_numpy(origins), to_numpy(directions), t_min, t_max, any_hit)

    def crossings(self, points, axis=2, below=True, n_tests=None):
        above, under, on = host_crossings(self.vertices, self.faces, to_numpy(points), axis)
        return above, (under if below else None), on

    def occlusion(self, points, normals, table, local=True, bias=0.0, t_max=np.inf, bits=False, n_tests=None):
        from .meshocclude import host_occlusion_rows
        return host_occlusion_rows(self.vertices, self.faces, to_numpy(points), to_numpy(normals), to_numpy(table), local, bias, t_max, bits)

    def project_rows(self, points, normals, images, views, hw=None, masks=None, bias=0.0, cos_min=0.0, weight='cosine', frame='raw',
                     bits=False, n_tests=None):
        from .meshproject import host_project_table
        return host_project_table(self.vertices, self.faces, to_numpy(points), to_numpy(normals), None if images is None else to_numpy(images),
                                  to_numpy(views), hw, None if masks is None else to_numpy(masks), bias, cos_min, weight, frame, bits)

    def contains(self, points, axis=2, vote=False):
        return _contains(self, points, axis, vote)


def _contains(mesh, points, axis, vote):
    """MeshIndex.contains / _HostMesh.contains: the parity of ``above``, or the majority of the three axes' parities."""
    if not vote:
        return (mesh.crossings(points, axis, below=False)[0] & 1) == 1
    votes = sum(mesh.crossings(points, a, below=False)[0] & 1 for a in range(3))
    return votes >= 2


def _prepare(mesh, device, name):
    """A mesh (anything meshcore.mesh_parts takes; a MeshIndex or _HostMesh is taken as it is) -> MeshIndex or _HostMesh.
    device='cpu' with device tensors: the caller asked for the host path."""
    if isinstance(mesh, (MeshIndex, _HostMesh)):
        return mesh
    v, f, _ = mesh_parts(mesh)
    if on_device(v, device):
        return MeshIndex(v, f, device=device, name=name)
    return _HostMesh(to_numpy(v), to_numpy(f), name)


def get_chamfer_dist(src_mesh, tgt_mesh, num_samples=10000, rng=None, device=None):
    """stage2/utils/metrics.py:79-101 (chamfer_dist.py:19-35 returns the first value only) -> (chamfer, raw): the mean distance
    of ``num_samples`` surface samples of each mesh to the other mesh, averaged over the two directions; raw = the samples and
    the per-sample distances under the reference's keys.  A mesh is anything with ``.vertices`` and ``.faces``.  Device tensors,
    or ``device='cuda'``, take the device path (raw then holds device tensors; nothing is copied back but the result);
    otherwise the host path.  ``rng``: np.random.RandomState (default: the global np.random, as the reference)."""
    src, tgt = _prepare(src_mesh, device, 'src_mesh'), _prepare(tgt_mesh, device, 'tgt_mesh')
    src_surf_pts, _ = src.sample_surface(num_samples, rng)
    tgt_surf_pts, _ = tgt.sample_surface(num_samples, rng)
    _, src_tgt_dist, _ = tgt.closest_point(src_surf_pts)
    _, tgt_src_dist, _ = src.closest_point(tgt_surf_pts)
    chamfer_dist = (src_tgt_dist.mean() + tgt_src_dist.mean()) / 2
    raw = {'tgt_surf_pts': tgt_surf_pts, 'src_surf_pts': src_surf_pts, 'src_tgt_dist': src_tgt_dist, 'tgt_src_dist': tgt_src_dist}
    return float(chamfer_dist), raw


def get_surface_dist(src_mesh, tgt_mesh, num_samples=10000, rng=None, device=None):
    """stage2/utils/metrics.py:103-113: the mean distance of ``num_samples`` surface samples of src_mesh to tgt_mesh."""
    src, tgt = _prepare(src_mesh, device, 'src_mesh'), _prepare(tgt_mesh, device, 'tgt_mesh')
    src_surf_pts, _ = src.sample_surface(num_samples, rng)
    _, src_tgt_dist, _ = tgt.closest_point(src_surf_pts)
    return float(src_tgt_dist.mean())
