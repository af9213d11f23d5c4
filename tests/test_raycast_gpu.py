"""Ray casting on the GPU (csrc/meshray.hip through psnerf_amd/meshdist.py and psnerf_amd/meshrender.py) against the float64 numpy
definition meshdist.host_ray_cast, on every mesh x ray set of tests/raycast_cases.py.

What is demanded, and why.  ``hit`` must be equal on EVERY ray: the intersection test is a fixed sequence of correctly rounded float64
+ - x / and comparisons, the same on both sides, with contraction off -- and the definition knows no grid, so the device's walk
through the grid may never lose a triangle.  A mismatch is a finding about the traversal or the order of operations, not a
tolerance to widen.  t is held to 1e-12 x the bounding-box diagonal, the project's float64 gate (see tests/test_chamfer_gpu.py).
Triangle ids are not compared directly (the count of equal ones is printed); instead the host's test of the ray against the
RETURNED triangle must reproduce the device's t and barycentrics.  The adversarial pairs are the point: the cube whose vertices
sit on the grid's corners with rays in its boundary planes, along its edges and through its corners, the oversize list, the flat
box, the one-triangle mesh.  A traversal that skips a cell fails there and nowhere else."""
import numpy as np
import pytest
import torch

from tests import raycast_cases as rc
from psnerf_amd import meshdist as md
from psnerf_amd import meshrender as mr

pytestmark = pytest.mark.gpu
GATE = 1e-12
MESHES = ['snapped cube', 'icosphere(2)', 'marching cubes', 'two oversize triangles', 'degenerate triangles', 'a single triangle',
          'flat bounding box']
_REFERENCE = {}


def mesh_case(name):
    """-> (vertices, faces, focus or None, rays per set)."""
    if name == 'snapped cube':
        v, f, n_cube = rc.snapped_cube(6)
        return v, f, (v[:n_cube].min(0), v[:n_cube].max(0)), 1500
    if name == 'icosphere(2)':
        return rc.icosphere(2) + (None, 1500)
    if name == 'marching cubes':
        return rc.mc_mesh() + (None, 500)
    return rc.awkward_meshes()[name] + (None, 1000)


def diagonal(v):
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def reference(name, index):
    """The ray sets of a mesh (laid along the grid ``index`` reports) with the definition's answer, computed once."""
    if name not in _REFERENCE:
        v, f, focus, count = mesh_case(name)
        sets = rc.ray_sets(v, f, index.lo, index.cell, index.n, count, seed=len(name), focus=focus)
        _REFERENCE[name] = dict((s, (o, d, t_min, t_max) + md.host_ray_cast(v, f, o, d, t_min, t_max)) for s, (o, d, t_min, t_max) in sets.items())
    return _REFERENCE[name]


def same(a, b):
    return all(torch.equal(x, y) or (x.dtype.is_floating_point and torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)))
               for x, y in zip(a, b))


@pytest.mark.parametrize('name', MESHES)
def test_device_against_the_definition(cuda, name):
    from psnerf_amd import hip
    v, f, focus, count = mesh_case(name)
    diag = diagonal(v)
    index = md.MeshIndex(v, f, device=cuda)
    again = md.MeshIndex(v, f, device=cuda)                      # (its lists may come out in another order)
    if name == 'snapped cube':                                   # the case is adversarial only while the vertices sit on the grid's corners
        n_cube = rc.snapped_cube(6)[2]
        k = (v[:n_cube] - np.asarray(index.lo)) / index.cell
        assert index.cell == rc.SNAP_CELL and index.n == [192, 192, 192] and index.lo == [rc.SNAP_LO] * 3
        assert np.array_equal(k, np.round(k)) and k.min() == rc.SNAP_FIRST and k.max() == rc.SNAP_FIRST + 6
        assert np.array_equal(np.asarray(index.lo) + k * index.cell, v[:n_cube])
    if name == 'two oversize triangles':
        assert index.n_over == 2
    if name == 'flat bounding box':
        assert index.n[2] == 1
    g = torch.Generator().manual_seed(0)
    for sname, (o, d, t_min, t_max, h_t, h_tri, h_bary, h_hit) in reference(name, index).items():
        what = '%s, %s' % (name, sname)
        od, dd = torch.from_numpy(o).to(cuda), torch.from_numpy(d).to(cuda)
        n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
        out = index.ray_cast(od, dd, t_min, t_max, n_tests=n_tests)
        assert same(out, again.ray_cast(od.clone(), dd.clone(), t_min, t_max)), what + ': two runs differ'
        # the order of the work changes nothing: a random permutation, and none
        raw = lambda order: hip.ray_cast(index.index, od, dd, t_min, t_max, order=order)
        plain = raw(None)
        assert same(plain, raw(torch.randperm(len(o), generator=g).to(cuda))), what + ': the order changes the result'
        assert same(out[:3], plain[:3]) and torch.equal(out[3], plain[3].bool())
        any_hit = index.ray_cast(od, dd, t_min, t_max, any_hit=True)[3]
        t, tri, bary, hit = (x.cpu().numpy() for x in out)
        per_ray = float(n_tests.item()) / len(o)
        print('%s: F=%d Q=%d hits %d (host %d), ids equal %d / %d, %.1f tests per ray' % (what, len(f), len(o), int(hit.sum()), int(h_hit.sum()),
                                                                                          int((tri == h_tri).sum()), len(o), per_ray))
        assert hit.dtype == np.bool_ and tri.dtype == np.int64 and np.array_equal(hit, h_hit), what + ': hit differs on %d rays' % int((hit != h_hit).sum())
        assert np.array_equal(any_hit.cpu().numpy(), h_hit), what + ': any-hit mode'
        assert np.array_equal(tri >= 0, hit) and tri.max() < len(f) and (t[~hit] == np.inf).all() and np.isnan(bary[~hit]).all()
        if hit.any():
            err = float(np.abs(t[hit] - h_t[hit]).max())
            r_t, r_bary, r_ok = md.host_ray_triangle(v, f, o, d, tri)
            err_tri = float(np.abs(r_t[hit] - t[hit]).max())
            err_bary = float(np.abs(r_bary[hit] - bary[hit]).max())
            print('    max |t - t_host| = %.3e, to the returned triangle %.3e, barycentrics %.3e (gate %.3e)' % (err, err_tri, err_bary, GATE * diag))
            assert r_ok[hit].all(), what + ': the host does not accept a returned triangle'
            assert err <= GATE * diag and err_tri <= GATE * diag and err_bary <= GATE, what
            assert ((t[hit] >= t_min) & (t[hit] <= t_max)).all()
        if name == 'degenerate triangles':
            assert (tri[hit] >= rc.N_REPEATED).all()


def test_no_cracks_on_the_device(cuda):
    """The icosphere(3): from 3 x every vertex, every edge midpoint and 2 000 surface samples, the ray toward the centre hits, between
    the inscribed sphere of the face planes and the unit sphere."""
    from tests.test_raycast_cpu import _centre_bound_origins
    v, f = rc.icosphere(3)
    r_in = rc.inner_radius(v, f)
    o = torch.from_numpy(_centre_bound_origins(v, f, 2000, 1)).to(cuda)
    assert len(o) == 642 + 1920 + 2000
    t, tri, bary, hit = md.MeshIndex(v, f, device=cuda).ray_cast(o, -o)
    assert bool(hit.all()) and bool((tri >= 0).all())
    r = (o + t[:, None] * (-o)).norm(dim=1)
    assert float(r.min()) >= r_in - 1e-12 and float(r.max()) <= 1.0 + 1e-12


def test_n_tests(cuda):
    """The two exact facts about the counter: a ray that misses the bounding box tests the oversize list and nothing else, and a camera
    bundle on the marching-cubes mesh stays below Q x F."""
    g = np.random.RandomState(5)
    unit = g.standard_normal((700, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    for name, n_over in (('two oversize triangles', 2), ('icosphere(2)', 0)):
        v, f = mesh_case(name)[:2]
        index = md.MeshIndex(v, f, device=cuda)
        assert index.n_over == n_over
        o = 4.0 * diagonal(v) * unit                               # outside the box, moving tangentially: never closer than 4 diagonals
        d = np.cross(o, g.standard_normal((700, 3)))
        n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
        hit = index.ray_cast(torch.from_numpy(o).to(cuda), torch.from_numpy(d).to(cuda), -np.inf, np.inf, n_tests=n_tests)[3]
        print('%s: %d rays that miss the box, %d tests (oversize list: %d)' % (name, len(o), int(n_tests.item()), n_over))
        assert not bool(hit.any()) and int(n_tests.item()) == n_over * len(o)
    v, f = rc.mc_mesh()
    index = md.MeshIndex(v, f, device=cuda)
    o, d, t_min, t_max = reference('marching cubes', index)['camera bundles'][:4]
    n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
    index.ray_cast(torch.from_numpy(o).to(cuda), torch.from_numpy(d).to(cuda), t_min, t_max, n_tests=n_tests)
    print('camera bundles on the marching-cubes mesh: %d tests for %d rays x %d faces' % (int(n_tests.item()), len(o), len(f)))
    assert 0 < int(n_tests.item()) < len(o) * len(f)


def test_public_layer_under_strict(cuda):
    """render_view at 64 x 48 and mesh_light_visibility with 300 points x 7 lights on the marching-cubes mesh: device path == host path
    (mask and visibility exactly, the maps within the gate), nothing falls back."""
    from psnerf_amd import ops
    from tests.test_raycast_cpu import _view
    v, f = rc.mc_mesh()
    diag = diagonal(v)
    H, W = 48, 64
    K, c2w = _view(H, W, fx=60.0, distance=3.0)
    g = np.random.RandomState(9)
    vn = g.standard_normal(v.shape)
    pts, _ = md.host_sample_surface(v, f, 300, g)
    lights = g.standard_normal((7, 3))
    host = mr.render_view((v, f), K, c2w, H, W)
    sv, sf = rc.icosphere(2)                                     # (interpolated vertex normals: on the small sphere, seen from the same camera)
    host_vn = mr.render_view((sv, sf), K, c2w, H, W, vertex_normals=vn[:len(sv)])
    host_vis = mr.mesh_light_visibility((v, f), pts, lights)
    ops.reset_hits()
    with ops.strict():
        index = md.MeshIndex(v, f, device=cuda)
        dev = mr.render_view(index, K.to(cuda), c2w.to(cuda), H, W)
        dev_vn = mr.render_view((sv, sf), K, c2w, H, W, vertex_normals=vn[:len(sv)], device=cuda)
        dev_vis = mr.mesh_light_visibility(index, torch.from_numpy(pts).to(cuda), torch.from_numpy(lights).to(cuda))
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    assert all(x.is_cuda for x in dev.values()) and dev_vis.is_cuda and dev_vis.shape == (7, 300) and dev_vis.dtype == torch.bool
    n_hit = int(host['mask'].sum())
    print('render_view 64 x 48: %d pixels on the mesh; visibility: %d of %d hidden' % (n_hit, int((~host_vis).sum()), host_vis.numel()))
    assert 100 < n_hit < H * W - 100 and 0 < int((~host_vis).sum()) < host_vis.numel()
    assert torch.equal(dev_vis.cpu(), host_vis)
    for a, b in ((dev, host), (dev_vn, host_vn)):
        assert torch.equal(a['mask'].cpu(), b['mask'])
        for key in ('t', 'depth', 'points', 'normals'):
            err = float((a[key].cpu() - b[key]).abs().max())
            print('    %s: max difference %.3e (gate %.3e)' % (key, err, GATE * diag))
            assert a[key].shape == b[key].shape and err <= GATE * diag


def test_c_abi_errors(cuda):
    from psnerf_amd import hip
    v, f = rc.icosphere(2)
    index = md.MeshIndex(v, f, device=cuda)
    o = torch.zeros(10, 3, dtype=torch.float64, device=cuda)
    d = torch.ones(10, 3, dtype=torch.float64, device=cuda)
    cast = lambda o, d, t_min=0.0, t_max=1.0: hip.ray_cast(index.index, o, d, t_min, t_max)
    assert bool(cast(o, d, 0.0, 3.0)[3].all())
    wide = torch.ones(10, 6, dtype=torch.float64, device=cuda)
    for bad in (lambda: cast(o.cpu(), d), lambda: cast(o, d.float()), lambda: cast(o, d, 2.0, 1.0), lambda: cast(o, d, float('nan'), 1.0),
                lambda: cast(wide[:, :3], d), lambda: cast(o, wide[:, ::2]), lambda: cast(o[:5], d)):
        with pytest.raises(RuntimeError, match='ray_cast'):
            bad()
    t, tri, bary, hit = cast(o[:0], d[:0])
    assert t.shape == (0,) and tri.shape == (0,) and bary.shape == (0, 3) and hit.shape == (0,) and t.is_cuda
