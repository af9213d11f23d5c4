"""Mesh evaluation without a GPU (psnerf_amd/meshdist.py): known answers of the point-to-triangle definition, the tie rule, the
surface sampler, the Chamfer distance between two icospheres, mesh files read back, the command-line tool on the host path, and the
argument validation of the new C entries."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import ROOT
from psnerf_amd import meshdist as md
from psnerf_amd.stage1.extracting import Mesh


def icosphere(radius, subdivisions=3):
    """An icosahedron subdivided ``subdivisions`` times, vertices on the sphere: 20 * 4^s faces (1280 at s = 3)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
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
    return Mesh(radius * np.asarray(v), np.asarray(f, dtype=np.int64))


TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float64)
TRI_F = np.array([[0, 1, 2]])


@pytest.mark.parametrize('z', [0.5, -0.5, 0.0])
def test_one_triangle_every_voronoi_region(z):
    cases = [((0.25, 0.25), (0.25, 0.25)),    # face
             ((-1.0, -1.0), (0.0, 0.0)),      # vertex A
             ((2.0, -0.5), (1.0, 0.0)),       # vertex B
             ((-0.5, 2.0), (0.0, 1.0)),       # vertex C
             ((0.5, -1.0), (0.5, 0.0)),       # edge AB
             ((-1.0, 0.5), (0.0, 0.5)),       # edge AC
             ((1.0, 1.0), (0.5, 0.5))]        # edge BC
    pts = np.array([[x, y, z] for (x, y), _ in cases])
    want = np.array([[x, y, 0.0] for _, (x, y) in cases])
    closest, dist, tri = md.host_closest_point(TRI_V, TRI_F, pts)
    assert closest.dtype == np.float64 and dist.dtype == np.float64 and tri.dtype == np.int64 and tri.tolist() == [0] * 7
    np.testing.assert_allclose(closest, want, rtol=0, atol=1e-15)
    np.testing.assert_allclose(dist, np.linalg.norm(pts - want, axis=1), rtol=0, atol=1e-15)
    # any corner order gives the same distances
    _, dist2, _ = md.host_closest_point(TRI_V, np.array([[2, 0, 1]]), pts)
    np.testing.assert_allclose(dist2, dist, rtol=0, atol=1e-15)


def unit_cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)   # index = 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int64)
    return v, f


def test_unit_cube_known_answers():
    v, f = unit_cube()
    assert f.shape == (12, 3)
    pts = np.array([[0.5, 0.5, 0.2], [0.5, 0.5, 1.5], [1.5, 1.5, 0.5], [2.0, 2.0, 2.0], [0.3, -0.25, 0.6]])
    closest, dist, tri = md.host_closest_point(v, f, pts)
    np.testing.assert_allclose(dist, [0.2, 0.5, 0.5 ** 0.5, 3.0 ** 0.5, 0.25], rtol=0, atol=1e-15)
    np.testing.assert_allclose(closest, [[0.5, 0.5, 0.0], [0.5, 0.5, 1.0], [1.0, 1.0, 0.5], [1.0, 1.0, 1.0], [0.3, 0.0, 0.6]], rtol=0, atol=1e-15)
    c2, d2 = md.host_point_triangle(v, f, pts, tri)
    assert np.array_equal(c2, closest) and np.array_equal(d2, dist)


def test_zero_area_triangles_are_segments_and_points():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 1, 1]], dtype=np.float64)
    pts = np.array([[1.5, 1.0, 0.0], [3.0, 0.0, 0.0], [-1.0, 0.0, 1.0], [0.5, 0.0, 0.0]])
    for order in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [0, 0, 2], [0, 2, 2]):   # collinear, also with a repeated corner
        closest, dist, _ = md.host_closest_point(v, np.array([order]), pts)
        assert np.isfinite(closest).all() and np.isfinite(dist).all(), order
        np.testing.assert_allclose(dist, [1.0, 1.0, 2.0 ** 0.5, 0.0], rtol=0, atol=1e-15, err_msg=str(order))
        np.testing.assert_allclose(closest, [[1.5, 0, 0], [2, 0, 0], [0, 0, 0], [0.5, 0, 0]], rtol=0, atol=1e-15, err_msg=str(order))
    closest, dist, _ = md.host_closest_point(v, np.array([[3, 3, 3]]), np.array([[1.0, 1.0, 3.0], [1.0, 1.0, 1.0]]))   # three equal points
    assert dist.tolist() == [2.0, 0.0] and closest.tolist() == [[1.0, 1.0, 1.0]] * 2
    # nearly collinear (area 5e-17): finite, and between the distances to the enclosing segment's ends
    v2 = np.array([[0, 0, 0], [1, 1e-16, 0], [2, 0, 0]], dtype=np.float64)
    _, dist, _ = md.host_closest_point(v2, TRI_F, pts)
    np.testing.assert_allclose(dist, [1.0, 1.0, 2.0 ** 0.5, 0.0], rtol=0, atol=1e-15)


def test_ties_go_to_the_lowest_triangle_index():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
    t0, t1 = [0, 1, 2], [1, 3, 2]
    p = np.array([[0.5, 0.5, 1.0], [0.75, 0.25, 2.0]])   # above the shared edge
    for faces in ([t0, t1], [t1, t0], [t1, t0, t0, t1]):
        _, dist, tri = md.host_closest_point(v, np.array(faces), p)
        assert tri.tolist() == [0, 0] and dist.tolist() == [1.0, 2.0]


def _barycentric(points, a, b, c):
    ab, ac, ap = b - a, c - a, points - a
    g11, g12, g22 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    r1, r2 = (ap * ab).sum(1), (ap * ac).sum(1)
    det = g11 * g22 - g12 * g12
    return (r1 * g22 - r2 * g12) / det, (r2 * g11 - r1 * g12) / det


def check_samples(vertices, faces, points, face_index, area_cum, seed, count):
    """The three sampler checks of one path (shared with tests/test_chamfer_gpu.py); all arguments numpy arrays."""
    diag = np.linalg.norm(vertices.max(0) - vertices.min(0))
    assert points.shape == (count, 3) and face_index.shape == (count,) and face_index.min() >= 0 and face_index.max() < len(faces)
    a, b, c = (vertices[faces[face_index, k]] for k in range(3))
    u, w = _barycentric(points, a, b, c)
    assert u.min() >= -1e-9 and w.min() >= -1e-9 and (u + w).max() <= 1.0 + 1e-9
    recon = (1.0 - u - w)[:, None] * a + u[:, None] * b + w[:, None] * c     # coordinates in [0, 1] that sum to 1
    assert np.abs(recon - points).max() <= 1e-12 * diag
    _, d = md.host_point_triangle(vertices, faces, points, face_index)       # on the closed triangle
    assert d.max() <= 1e-12 * diag
    pick = np.random.RandomState(seed).random_sample(count)
    want = np.minimum(np.searchsorted(area_cum, pick * area_cum[-1]), len(faces) - 1)
    assert np.array_equal(face_index, want)


def test_sampler_on_an_icosphere():
    m = icosphere(1.0)
    assert m.faces.shape[0] >= 1280
    pts, fi, cum = md.host_sample_surface(m.vertices, m.faces, 5000, np.random.RandomState(3), return_cumulative=True)
    assert pts.dtype == np.float64 and fi.dtype == np.int64
    assert np.allclose(cum, np.cumsum(md.host_face_areas(m.vertices, m.faces)), rtol=1e-15)
    check_samples(m.vertices, m.faces, pts, fi, cum, 3, 5000)
    # default rng = the global np.random, as the reference
    np.random.seed(11)
    p1, _ = md.host_sample_surface(m.vertices, m.faces, 10)
    p2, _ = md.host_sample_surface(m.vertices, m.faces, 10, np.random.RandomState(11))
    assert np.array_equal(p1, p2)


def two_triangles_1_to_3():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [6, 0, 1], [0, 1, 1]], dtype=np.float64)
    return v, np.array([[0, 1, 2], [3, 4, 5]])


def test_sampler_area_shares():
    v, f = two_triangles_1_to_3()
    assert md.host_face_areas(v, f).tolist() == [1.0, 3.0]
    _, fi = md.host_sample_surface(v, f, 40000, np.random.RandomState(0))
    share = float((fi == 1).mean())
    sigma = (0.75 * 0.25 / 40000) ** 0.5
    print('share of the large triangle: %.5f (0.75 +- %.5f)' % (share, 5 * sigma))
    assert abs(share - 0.75) <= 5 * sigma


def test_chamfer_between_two_icospheres():
    a, b = icosphere(1.0), icosphere(1.1)
    ch_ab, raw = md.get_chamfer_dist(a, b, 10000, rng=np.random.RandomState(1))
    ch_ba, _ = md.get_chamfer_dist(b, a, 10000, rng=np.random.RandomState(2))
    print('chamfer(1.0, 1.1) = %.6f, swapped %.6f' % (ch_ab, ch_ba))
    assert 0.09 < ch_ab < 0.11 and 0.09 < ch_ba < 0.11
    # symmetric to the sampling noise: each one-sided mean is a mean of 10 000 distances whose spread is below 0.01
    assert abs(ch_ab - ch_ba) < 5 * 0.01 / 10000 ** 0.5
    assert sorted(raw) == ['src_surf_pts', 'src_tgt_dist', 'tgt_src_dist', 'tgt_surf_pts']
    assert raw['src_surf_pts'].shape == raw['tgt_surf_pts'].shape == (10000, 3) and raw['src_tgt_dist'].shape == raw['tgt_src_dist'].shape == (10000,)
    assert np.allclose(np.linalg.norm(raw['tgt_surf_pts'], axis=1), 1.1, atol=0.01) and raw['src_tgt_dist'].std() < 0.01
    assert ch_ab == (raw['src_tgt_dist'].mean() + raw['tgt_src_dist'].mean()) / 2
    assert md.get_surface_dist(a, a, 2000, rng=np.random.RandomState(5)) < 1e-12
    # the re-exports with the reference's names
    from psnerf_amd import metrics
    ch2, _ = metrics.get_chamfer_dist(a, b, 10000, rng=np.random.RandomState(1))
    assert ch2 == ch_ab and metrics.get_surface_dist(a, a, 100, rng=np.random.RandomState(5)) < 1e-12


def test_empty_mesh_is_named():
    a = icosphere(1.0, 1)
    empty = Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(ValueError, match='tgt_mesh'):
        md.get_chamfer_dist(a, empty, 10, rng=np.random.RandomState(0))
    with pytest.raises(ValueError, match='src_mesh'):
        md.get_surface_dist(empty, a, 10, rng=np.random.RandomState(0))
    with pytest.raises(ValueError):
        md.host_closest_point(a.vertices, np.array([[0, 1, 99999]]), np.zeros((1, 3)))


def test_load_mesh_round_trips(tmp_path):
    m = icosphere(1.0 / 3.0, 2)
    normals = m.vertices / np.linalg.norm(m.vertices, axis=1, keepdims=True)
    for with_n in (False, True):
        mesh = Mesh(m.vertices, m.faces, vertex_normals=normals.astype(np.float32) if with_n else None)
        p = mesh.export(str(tmp_path / ('m%d.obj' % with_n)))
        back = md.load_mesh(p)
        assert np.array_equal(back.vertices, m.vertices) and np.array_equal(back.faces, m.faces)      # %.17g: bit-equal
        assert (back.vertex_normals is not None) == with_n
        p = mesh.export(str(tmp_path / ('m%d.ply' % with_n)))
        back = md.load_mesh(p)
        assert np.array_equal(back.vertices.astype(np.float32), m.vertices.astype(np.float32)) and np.array_equal(back.faces, m.faces)
        assert back.vertices.dtype == np.float64 and back.faces.dtype == np.int64
        if with_n:
            assert np.array_equal(back.vertex_normals.astype(np.float32), normals.astype(np.float32))
    # ASCII .ply with a quad, a comment and an extra vertex property
    p = tmp_path / 'a.ply'
    p.write_text('ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 5\nproperty double x\nproperty double y\nproperty double z\n'
                 'property uchar red\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n'
                 '0 0 0 255\n1 0 0 255\n1 1 0 0\n0 1 0 0\n0.5 0.5 1 7\n4 0 1 2 3\n3 0 1 4\n')
    back = md.load_mesh(str(p))
    assert back.vertices.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]]
    assert back.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]
    # binary .ply with faces of different sizes (the general path)
    import struct
    p = tmp_path / 'b.ply'
    head = 'ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 2\n' \
           'property list uchar uint vertex_index\nend_header\n'
    body = struct.pack('<12f', 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0) + struct.pack('<B3I', 3, 0, 1, 2) + struct.pack('<B4I', 4, 0, 1, 2, 3)
    p.write_bytes(head.encode('ascii') + body)
    assert md.load_mesh(str(p)).faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3]]
    # .obj with a/b/c corners, a quad, and indices relative to the end
    p = tmp_path / 'c.obj'
    p.write_text('# hand made\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1 4/1/1\nf 1/1 2/1 3/1\nf -4 -3 -1\n')
    back = md.load_mesh(str(p))
    assert back.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 1, 3]] and back.vertex_normals is None
    # anything else raises with the file name
    p = tmp_path / 'd.stl'
    p.write_text('solid\n')
    with pytest.raises(ValueError, match='d.stl'):
        md.load_mesh(str(p))
    p = tmp_path / 'e.ply'
    p.write_text('ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n')
    with pytest.raises(ValueError, match='e.ply'):
        md.load_mesh(str(p))
    p = tmp_path / 'f.obj'
    p.write_text('v 0 0 0\nf 1 2 3\n')
    with pytest.raises(ValueError, match='f.obj'):
        md.load_mesh(str(p))


def test_command_line_tool_on_the_host_path(tmp_path):
    a = icosphere(1.0, 2).export(str(tmp_path / 'gt.ply'))
    b = icosphere(1.1, 2).export(str(tmp_path / 'pred.obj'))
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, 'tools', 'chamfer_dist.py'), '--mesh_gt', a, '--mesh_pred', b,
                                   '--num_samples', '2000', '--seed', '0', '--no-cuda']).decode()
    lines = [l for l in out.splitlines() if l.startswith('Chamfer')]
    assert len(lines) == 1 and re.match(r'^Chamfer Distance \(mm\):  \d+\.\d\d$', lines[0]), out
    assert 85.0 < float(lines[0].split()[-1]) < 115.0


def test_argument_validation_of_the_mesh_distance_entries_needs_no_gpu():
    from psnerf_amd import hip
    lib = hip._lib
    dummy = ctypes.c_void_p(64)
    g = hip.tri_grid([0, 0, 0], [1, 1, 1], 0.25, [4, 4, 4], 256)
    assert ctypes.sizeof(hip.PsnTriGrid) == 72
    rc = lib.psn_tri_grid_count(None, dummy, dummy, 1, dummy, dummy, dummy, None)
    assert rc == -1 and b'null grid' in lib.psn_last_error()
    rc = lib.psn_tri_grid_count(ctypes.byref(g), None, dummy, 1, dummy, dummy, dummy, None)
    assert rc == -1 and b'null pointer' in lib.psn_last_error()
    rc = lib.psn_tri_grid_count(ctypes.byref(g), dummy, dummy, 0, dummy, dummy, dummy, None)
    assert rc == -1 and b'n_faces' in lib.psn_last_error()
    rc = lib.psn_tri_grid_fill(ctypes.byref(g), dummy, dummy, 5, dummy, 1 << 31, dummy, None)
    assert rc == -1 and b'n_entries' in lib.psn_last_error()
    rc = lib.psn_tri_grid_fill(ctypes.byref(g), dummy, dummy, 5, None, 10, dummy, None)
    assert rc == -1 and b'null pointer' in lib.psn_last_error()
    assert ctypes.sizeof(hip.PsnMeshIndex) == 128

    def index(grid=g, n_over=0):
        ix = hip.PsnMeshIndex()
        ix.grid, ix.vertices, ix.faces, ix.n_faces, ix.cell_start, ix.list, ix.over_list, ix.n_over = grid, 64, 64, 5, 64, 64, 64, n_over
        return ctypes.byref(ix)
    rc = lib.psn_closest_point(index(n_over=6), dummy, None, 3, dummy, dummy, dummy, None, None)
    assert rc == -1 and b'n_over' in lib.psn_last_error()
    rc = lib.psn_closest_point(index(), None, None, 3, dummy, dummy, dummy, None, None)
    assert rc == -1 and b'null point' in lib.psn_last_error()
    rc = lib.psn_closest_point(index(), dummy, None, -1, dummy, dummy, dummy, None, None)
    assert rc == -1 and b'n_points' in lib.psn_last_error()
    assert lib.psn_closest_point(index(), None, None, 0, None, None, None, None, None) == 0   # Q = 0: a no-op
    # the four queries after the index, with otherwise valid arguments: a null index and (below) a bad grid are the first thing refused
    queries = ((lib.psn_closest_point, (dummy, None, 3, dummy, dummy, dummy, None, None)),
               (lib.psn_ray_cast, (dummy, dummy, None, 3, 0.0, 1.0, hip.RAY_FIRST_HIT, dummy, dummy, dummy, dummy, None, None)),
               (lib.psn_mesh_crossings, (dummy, None, 3, 2, dummy, dummy, dummy, None, None)),
               (lib.psn_occlusion_rows, (dummy, dummy, 3, dummy, 4, hip.OCC_LOCAL, 0.0, 1.0, dummy, dummy, dummy, dummy, dummy, None, None)))
    for fn, rest in queries:
        assert fn(None, *rest) == -1 and b'null' in lib.psn_last_error(), lib.psn_last_error()
    for bad, word in ((dict(cell=0.0), b'cell size'), (dict(cell=float('nan')), b'cell size'), (dict(n=[4, 0, 4]), b'cells on axis 1'),
                      (dict(n=[4, 4, 257]), b'cells on axis 2'), (dict(lo=[0, 2, 0]), b'bounding box'),
                      (dict(hi=[1, float('inf'), 1]), b'bounding box'), (dict(max_span=0), b'max_span')):
        kw = dict(lo=[0, 0, 0], hi=[1, 1, 1], cell=0.25, n=[4, 4, 4], max_span=256)
        kw.update(bad)
        b = hip.tri_grid(**kw)
        for fn, rest in ((lib.psn_tri_grid_count, (dummy, dummy, 1, dummy, dummy, dummy, None)),
                         (lib.psn_tri_grid_fill, (dummy, dummy, 1, dummy, 1, dummy, None))):
            rc = fn(ctypes.byref(b), *rest)
            assert rc == -1 and word in lib.psn_last_error(), (bad, lib.psn_last_error())
        for fn, rest in queries:
            rc = fn(index(grid=b), *rest)
            assert rc == -1 and word in lib.psn_last_error(), (bad, lib.psn_last_error())
    # the wrappers refuse host tensors: there is no host fall-back behind them
    import torch
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        hip.mesh_index(g, torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(65, dtype=torch.int32),
                       torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 0)
