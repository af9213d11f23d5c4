"""Mesh evaluation on the GPU (csrc/meshdist.hip through psnerf_amd/meshdist.py) against the float64 numpy definition in the same
module: the distance query on marching-cubes meshes and on awkward ones, the sampler, the Chamfer distance device vs host, and the
shipped extraction size under ops.strict().

The gate of every distance comparison is 1e-12 x the bounding-box diagonal of the mesh, the project's float64 gate
(tests/test_mesh_gpu.py): the definition differs from the same formulas in 80-bit arithmetic by some 1e-16 x diagonal, a device
that rounds a multiply-add differently is of that order.  Triangle ids are not compared across the two paths (a last-bit difference
may flip a near-tie); instead the host distance from the query to the RETURNED triangle must equal the returned distance."""
import types

import numpy as np
import pytest
import torch

from tests import mesh_fields as mf
from tests.test_chamfer_cpu import check_samples
from psnerf_amd import meshdist as md

pytestmark = pytest.mark.gpu
GATE = 1e-12
_MESHES = {}


def mc_mesh(R):
    """The marching-cubes mesh of the sphere + rod + torus field at resolution R, in world units (host path)."""
    if R not in _MESHES:
        from psnerf_amd.stage1.extracting import host_marching_cubes, to_world
        v, f = host_marching_cubes(mf.sphere_rod_torus(R), 0.0)
        _MESHES[R] = (to_world(v, R + 1, mf.BOX_SIZE), f)
    return _MESHES[R]


def diagonal(v):
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def check_against_host(cuda, v, f, queries, what, **grid):
    """MeshIndex.closest_point against host_closest_point; two device runs bit-identical.  Returns the device distances.
    ``grid``: MeshIndex's ``cell`` / ``max_span``, for a grid other than the default one."""
    diag = diagonal(v)
    index = md.MeshIndex(v, f, device=cuda, **grid)
    pts = torch.from_numpy(queries).to(cuda)
    closest, dist, tri = index.closest_point(pts)
    c2, d2, t2 = md.MeshIndex(v, f, device=cuda, **grid).closest_point(pts.clone())
    assert torch.equal(closest, c2) and torch.equal(dist, d2) and torch.equal(tri, t2), what + ': two runs differ'
    closest, dist, tri = closest.cpu().numpy(), dist.cpu().numpy(), tri.cpu().numpy()
    assert tri.dtype == np.int64 and tri.min() >= 0 and tri.max() < len(f)
    _, h_dist, h_tri = md.host_closest_point(v, f, queries)
    err = float(np.abs(dist - h_dist).max()) if len(queries) else 0.0
    hc, hd = md.host_point_triangle(v, f, queries, tri)            # the host's answer for the triangle the device returned
    err_tri = float(np.abs(hd - dist).max())
    err_pt = float(np.abs(hc - closest).max())
    err_at = float(np.abs(np.linalg.norm(queries - closest, axis=1) - dist).max())
    print('%s: F=%d Q=%d cells=%s lists=%d oversize=%d | max |d - d_host| = %.3e, to the returned triangle %.3e, closest point %.3e, '
          '| |q - closest| - d | = %.3e (gate %.3e); ids equal: %d / %d'
          % (what, len(f), len(queries), index.n, index.n_entries, index.n_over, err, err_tri, err_pt, err_at, GATE * diag,
             int((tri == h_tri).sum()), len(tri)))
    assert err <= GATE * diag, what
    assert err_tri <= GATE * diag and err_pt <= GATE * diag and err_at <= GATE * diag, what
    return dist


def query_sets(R, n=2000):
    v, f = mc_mesh(R)
    ov, of = mc_mesh(96 - R)
    g = np.random.RandomState(R)
    lo, hi = v.min(0), v.max(0)
    other, _ = md.host_sample_surface(ov, of, n, g)
    return {'uniform in the box': lo + g.random_sample((n, 3)) * (hi - lo),
            'mesh vertices': v[g.choice(len(v), n, replace=False)],
            'samples of the other mesh': other,
            'uniform in +-10': (g.random_sample((n, 3)) - 0.5) * 20.0}


@pytest.mark.parametrize('R,n_faces', [(32, 5728), (64, 22816)])
def test_closest_point_on_marching_cubes_meshes(cuda, R, n_faces):
    v, f = mc_mesh(R)
    assert len(f) == n_faces and abs(diagonal(v) - 3.25) < 0.01 and md.host_face_areas(v, f).min() > 0
    for name, q in query_sets(R).items():
        dist = check_against_host(cuda, v, f, q, 'R=%d, %s' % (R, name))
        if name == 'mesh vertices':
            assert dist.max() <= GATE * diagonal(v)


def test_closest_point_robustness(cuda):
    v, f = mc_mesh(32)
    g = np.random.RandomState(7)
    lo, hi = v.min(0), v.max(0)
    q = np.concatenate([lo + g.random_sample((700, 3)) * (hi - lo), (g.random_sample((700, 3)) - 0.5) * 24.0, v[:600]])
    # two triangles that span a box ten times the mesh's
    big = 10.0 * np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]], [hi[0], hi[1], lo[2]]])
    v2 = np.concatenate([v, big])
    f2 = np.concatenate([f, len(v) + np.array([[0, 1, 2], [1, 3, 2]])])
    index = md.MeshIndex(v2, f2, device=cuda)
    assert index.n_over == 2 and index.n_entries < 64 * len(f2)          # kept aside: the cell lists do not explode
    check_against_host(cuda, v2, f2, q, 'mesh + two spanning triangles')
    # duplicated and zero-area triangles appended
    dup = f[g.choice(len(f), 300, replace=False)]
    zero = np.stack([dup[:100, 0], dup[:100, 1], dup[:100, 1]], axis=1)            # a repeated corner: a segment
    point = np.repeat(f[:50, :1], 3, axis=1)                                        # three equal corners: a point
    mid = np.concatenate([v, 0.5 * (v[f[:80, 0]] + v[f[:80, 1]])])                  # a collinear triple: a, midpoint, b
    coll = np.stack([f[:80, 0], len(v) + np.arange(80), f[:80, 1]], axis=1)
    f3 = np.concatenate([f, dup, zero, point, coll])
    check_against_host(cuda, mid, f3, q, 'duplicated and zero-area triangles')
    # a single triangle
    tv = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.5, 0.9]])
    check_against_host(cuda, tv, np.array([[0, 1, 2]]), (g.random_sample((1500, 3)) - 0.5) * 6.0, 'a single triangle')
    # a flat bounding box (all z equal)
    fv = v.copy()
    fv[:, 2] = 0.25
    check_against_host(cuda, fv, f, q, 'flat bounding box')
    # Q = 0 returns empty tensors; F = 0 raises
    index = md.MeshIndex(v, f, device=cuda)
    c, d, t = index.closest_point(torch.zeros(0, 3, dtype=torch.float64, device=cuda))
    assert c.shape == (0, 3) and d.shape == (0,) and t.shape == (0,) and t.dtype == torch.int64 and c.is_cuda
    with pytest.raises(ValueError, match='empty'):
        md.MeshIndex(v, np.zeros((0, 3), dtype=np.int64), device=cuda)
    with pytest.raises(ValueError, match='refers to vertex'):
        md.MeshIndex(v, np.array([[0, 1, len(v)]]), device=cuda)
    # a NaN query is at no distance; its neighbours are untouched
    qn = torch.from_numpy(q[:3].copy()).to(cuda)
    qn[1, 0] = float('nan')
    c, d, t = index.closest_point(qn)
    c0, d0, t0 = index.closest_point(torch.from_numpy(q[:3].copy()).to(cuda))
    assert bool(torch.isnan(d[1])) and int(t[1]) == -1 and torch.equal(d[[0, 2]], d0[[0, 2]]) and torch.equal(t[[0, 2]], t0[[0, 2]])


def test_sampler_on_the_device(cuda):
    for v, f, count, seed in (mc_mesh(32) + (5000, 3), mc_mesh(64) + (5000, 4)):
        index = md.MeshIndex(v, f, device=cuda)
        pts, fi, cum = index.sample_surface(count, np.random.RandomState(seed), return_cumulative=True)
        assert pts.is_cuda and pts.dtype == torch.float64 and fi.dtype == torch.int64
        cum = cum.cpu().numpy()
        check_samples(v, f, pts.cpu().numpy(), fi.cpu().numpy(), cum, seed, count)
        ref = np.cumsum(md.host_face_areas(v, f))
        rel = float(np.abs(cum / ref - 1.0).max())
        print('cumulative areas, device vs numpy: max relative difference %.3e' % rel)
        assert rel <= 1e-12
    from tests.test_chamfer_cpu import two_triangles_1_to_3
    v, f = two_triangles_1_to_3()
    _, fi = md.MeshIndex(v, f, device=cuda).sample_surface(40000, np.random.RandomState(0))
    share = float((fi == 1).double().mean())
    assert abs(share - 0.75) <= 5 * (0.75 * 0.25 / 40000) ** 0.5


def test_chamfer_device_against_host(cuda):
    a = types.SimpleNamespace(vertices=mc_mesh(32)[0], faces=mc_mesh(32)[1])
    b = types.SimpleNamespace(vertices=mc_mesh(64)[0], faces=mc_mesh(64)[1])
    diag = max(diagonal(a.vertices), diagonal(b.vertices))
    n = 10000
    ch_h, raw_h = md.get_chamfer_dist(a, b, n, rng=np.random.RandomState(5))
    ch_d, raw_d = md.get_chamfer_dist(a, b, n, rng=np.random.RandomState(5), device=cuda)
    assert all(torch.is_tensor(x) and x.is_cuda for x in raw_d.values()) and sorted(raw_d) == sorted(raw_h)
    raw_d = dict((k, x.cpu().numpy()) for k, x in raw_d.items())
    # a face pick within rounding of a cumulative-area boundary may differ between the paths: such samples are excluded, at most 0.1 %
    keep = {}
    g_h, g_d = np.random.RandomState(5), np.random.RandomState(5)      # the same draws once more, for the face indices
    for side, m in (('src', a), ('tgt', b)):
        p_h, fi_h = md.host_sample_surface(m.vertices, m.faces, n, g_h)
        p_d, fi_d = md.MeshIndex(m.vertices, m.faces, device=cuda).sample_surface(n, g_d)
        assert np.array_equal(p_h, raw_h[side + '_surf_pts']) and np.array_equal(p_d.cpu().numpy(), raw_d[side + '_surf_pts'])
        same = fi_d.cpu().numpy() == fi_h
        print('%s samples whose face index differs between the paths: %d of %d' % (side, int((~same).sum()), n))
        assert (~same).sum() <= n // 1000
        assert np.abs(raw_d[side + '_surf_pts'] - raw_h[side + '_surf_pts'])[same].max() <= GATE * diag
        keep[side] = same
    m_h = [raw_h['src_tgt_dist'][keep['src']].mean(), raw_h['tgt_src_dist'][keep['tgt']].mean()]
    m_d = [raw_d['src_tgt_dist'][keep['src']].mean(), raw_d['tgt_src_dist'][keep['tgt']].mean()]
    print('one-sided means host %r device %r; chamfer host %.17g device %.17g' % (m_h, m_d, ch_h, ch_d))
    assert abs(m_h[0] - m_d[0]) <= GATE * diag and abs(m_h[1] - m_d[1]) <= GATE * diag
    assert abs((m_h[0] + m_h[1]) / 2 - (m_d[0] + m_d[1]) / 2) <= GATE * diag
    if keep['src'].all() and keep['tgt'].all():
        assert abs(ch_h - ch_d) <= GATE * diag
    # device tensors in -> the device path without being asked; the one-sided distance too
    da = types.SimpleNamespace(vertices=torch.from_numpy(a.vertices).to(cuda), faces=torch.from_numpy(a.faces).to(cuda))
    db = md.MeshIndex(b.vertices, b.faces, device=cuda)        # an index is a mesh too, and is not rebuilt
    ch_d2, raw_d2 = md.get_chamfer_dist(da, db, n, rng=np.random.RandomState(5))
    assert ch_d2 == ch_d and raw_d2['src_tgt_dist'].is_cuda
    s_h = md.get_surface_dist(a, b, 3000, rng=np.random.RandomState(6))
    s_d = md.get_surface_dist(da, db, 3000, rng=np.random.RandomState(6))
    assert abs(s_h - s_d) <= GATE * diag
    with pytest.raises(ValueError, match='tgt_mesh'):
        md.get_chamfer_dist(a, types.SimpleNamespace(vertices=np.zeros((0, 3)), faces=np.zeros((0, 3), dtype=np.int64)), 10, device=cuda)


def test_shipped_size_under_strict(cuda):
    """The sphere-initialised BEAR network of tools/bench_mesh.py extracted at (64, 3) and at (64, 2) on the device; Chamfer between the
    two with 10 000 samples, meshes and samples on the device throughout.  64 of the queries against the fine mesh (every 156th)
    are checked against the host definition (64 x 683 k float64 pair tests); the self-distance of 100 000 surface samples of the
    fine mesh covers every query of a large run: a sample is a float64 combination of its face's corners, so its true distance
    to the mesh is the rounding of that combination (order 1e-16 x diagonal), to which the device may add the gate."""
    from psnerf_amd import hip, ops
    import psnerf_amd.stage1 as s1
    from psnerf_amd.stage1.extracting import Extractor3D, iso_value
    from psnerf_amd.synthetic import stage1_cfg
    torch.manual_seed(0)
    net = s1.NeuralNetwork(stage1_cfg('bear')).to(cuda)
    ops.reset_hits()
    with ops.strict():
        meshes = []
        for steps in (3, 2):
            ex = Extractor3D(net, device=cuda, resolution0=64, upsampling_steps=steps)
            ex.generate_mesh()
            v, f = hip.marching_cubes(ex.last_grid.contiguous(), iso_value(ex.threshold), 2 + ex.padding)
            meshes.append(md.MeshIndex(v, f, name='mesh (64, %d)' % steps))
        fine, coarse = meshes
        n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
        chamfer, raw = md.get_chamfer_dist(fine, coarse, 10000, rng=np.random.RandomState(0))
        _, d_again, _ = fine.closest_point(raw['tgt_surf_pts'], n_tests=n_tests)
        self_pts, _ = fine.sample_surface(100000, np.random.RandomState(1))
        _, self_dist, _ = fine.closest_point(self_pts)
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    assert all(x.is_cuda for x in raw.values()) and torch.equal(d_again, raw['tgt_src_dist'])
    fv, ff = fine.vertices.cpu().numpy(), fine.faces.cpu().numpy()
    diag = diagonal(fv)
    per_query = float(n_tests.item()) / 10000
    print('fine mesh: %d faces, %s cells, %d list entries, %d oversize, index %.1f MB; coarse mesh: %d faces; chamfer %.6e; '
          '%.1f triangle tests per query (F / 100 = %.0f)' % (len(ff), fine.n, fine.n_entries, fine.n_over, fine.index_bytes / 1e6,
                                                              coarse.faces.shape[0], chamfer, per_query, len(ff) / 100.0))
    assert len(ff) > 100000 and 0.0 < chamfer < 0.01 * diag
    assert per_query < len(ff) / 100.0
    pick = np.arange(0, 10000, 156)[:64]
    q = raw['tgt_surf_pts'].cpu().numpy()[pick]
    _, h_dist, _ = md.host_closest_point(fv, ff, q)
    err = float(np.abs(raw['tgt_src_dist'].cpu().numpy()[pick] - h_dist).max())
    worst = float(self_dist.max())
    print('64 queries against the host definition: max |d - d_host| = %.3e (gate %.3e); self-distance of 100 000 samples: max %.3e '
          '(gate %.3e)' % (err, GATE * diag, worst, 2 * GATE * diag))
    assert err <= GATE * diag
    assert worst <= 2 * GATE * diag
