"""The definition of ray casting (psnerf_amd/meshdist.py:host_ray_cast, the watertight test of Woop, Benthin and Wald) and the host
path of psnerf_amd/meshrender.py.  No device.  Every bound below follows from the construction (known answers, convexity, the
analytic sphere); nothing is measured."""
import numpy as np
import torch

from tests import raycast_cases as rc
from psnerf_amd import meshdist as md
from psnerf_amd import meshrender as mr


def test_known_answers():
    # one triangle in the plane z = 1; a ray from the origin through (0.25, 0.5, 1): t = 1 along d = (0.25, 0.5, 1); the point is
    # a + 0.25 (b - a) + 0.5 (c - a), so the barycentrics are (0.25, 0.25, 0.5)
    v = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    f = np.array([[0, 1, 2]])
    t, tri, bary, hit = md.host_ray_cast(v, f, [[0.0, 0.0, 0.0]], [[0.25, 0.5, 1.0]])
    assert hit[0] and tri[0] == 0 and t[0] == 1.0 and np.array_equal(bary[0], [0.25, 0.25, 0.5])
    t, tri, bary, hit = md.host_ray_cast(v, f, [[0.0, 0.0, 0.0]], [[0.5, 1.0, 2.0]])          # the same ray, d twice as long
    assert hit[0] and t[0] == 0.5 and np.array_equal(bary[0], [0.25, 0.25, 0.5])
    for d in ([-0.25, 0.5, 1.0], [0.25, 0.5, -1.0], [0.8, 0.8, 1.0]):                         # beside, behind, beyond the hypotenuse
        assert not md.host_ray_cast(v, f, [[0.0, 0.0, 0.0]], [d])[3][0]
    # from behind (no back-face culling), and the window on t
    assert md.host_ray_cast(v, f, [[0.25, 0.5, 3.0]], [[0.0, 0.0, -1.0]])[0][0] == 2.0
    assert not md.host_ray_cast(v, f, [[0.25, 0.5, 3.0]], [[0.0, 0.0, -1.0]], t_min=2.5)[3][0]
    assert not md.host_ray_cast(v, f, [[0.25, 0.5, 3.0]], [[0.0, 0.0, -1.0]], t_max=1.5)[3][0]
    assert md.host_ray_cast(v, f, [[0.25, 0.5, 3.0]], [[0.0, 0.0, -1.0]], t_min=2.0, t_max=2.0)[3][0]
    # two triangles that share the edge (1, 0, 1) - (0, 1, 1): rays exactly through the edge and exactly through a shared vertex hit,
    # and the tie goes to the lower id, whichever way the faces are listed
    v2 = np.concatenate([v, [[1.0, 1.0, 1.0]]])
    for f2 in (np.array([[0, 1, 2], [1, 3, 2]]), np.array([[1, 3, 2], [0, 1, 2]])):
        for target in ([0.5, 0.5, 1.0], [0.25, 0.75, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]):
            for o in ([0.0, 0.0, 0.0], [0.3, -0.2, -1.0], [0.5, 0.5, 4.0]):
                d = np.asarray(target) - np.asarray(o)
                t, tri, bary, hit = md.host_ray_cast(v2, f2, [o], [d])
                assert hit[0] and tri[0] == 0 and t[0] == 1.0, (f2.tolist(), target, o)
                both = md.host_ray_triangle(v2, f2, [o, o], [d, d], [0, 1])
                assert both[2].all() and both[0][0] == both[0][1] == 1.0
    # a miss is (inf, -1, NaN, False); an empty mesh and a reversed window are refused
    t, tri, bary, hit = md.host_ray_cast(v, f, [[5.0, 5.0, 0.0]], [[0.0, 0.0, 1.0]])
    assert t[0] == np.inf and tri[0] == -1 and np.isnan(bary[0]).all() and not hit[0]
    for bad in (lambda: md.host_ray_cast(v, np.zeros((0, 3), dtype=np.int64), [[0, 0, 0]], [[0, 0, 1]]),
                lambda: md.host_ray_cast(v, f, [[0, 0, 0]], [[0, 0, 1]], t_min=2.0, t_max=1.0)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError('no ValueError')


def _centre_bound_origins(v, f, n_random, seed):
    g = np.random.RandomState(seed)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    pts, _ = md.host_sample_surface(v, f, n_random, g)
    return 3.0 * np.concatenate([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]]), pts])


def test_no_cracks_on_the_icosphere():
    """From every origin o = 3 x (vertex | edge midpoint | surface sample) the ray toward the centre hits, and the hit point lies
    between the inscribed sphere of the face planes and the unit sphere: the mesh is closed and convex and contains the centre."""
    v, f = rc.icosphere(2)
    r_in = rc.inner_radius(v, f)
    assert 0.9 < r_in < 1.0
    o = _centre_bound_origins(v, f, 2000, 0)
    assert len(o) == 162 + 480 + 2000
    t, tri, bary, hit = md.host_ray_cast(v, f, o, -o)
    assert hit.all() and (tri >= 0).all()
    r = np.linalg.norm(o + t[:, None] * (-o), axis=1)
    assert r.min() >= r_in - 1e-12 and r.max() <= 1.0 + 1e-12, (r.min(), r.max(), r_in)
    assert np.abs(bary.sum(1) - 1.0).max() <= 1e-15 * 4 and bary.min() >= 0.0
    # the returned triangle reproduces the returned t; the any-hit mode agrees with the first-hit mode
    t2, bary2, ok = md.host_ray_triangle(v, f, o, -o, tri)
    assert ok.all() and np.array_equal(t2, t) and np.array_equal(bary2, bary)
    assert md.host_ray_cast(v, f, o, -o, any_hit=True)[3].all()


def test_every_ray_set_on_the_awkward_meshes():
    """host_ray_triangle reproduces t for the returned triangle; triangles with a repeated corner are never returned; any_hit == hit;
    rays with a NaN, an infinity or a zero direction miss."""
    for name, (v, f) in rc.awkward_meshes().items():
        lo, hi = v.min(0), v.max(0)
        cell = max(float((hi - lo).max()) / 16.0, 1e-3)
        n = np.maximum(1, np.ceil((hi - lo) / cell)).astype(int)
        for sname, (o, d, t_min, t_max) in rc.ray_sets(v, f, lo, cell, n, 150, seed=3).items():
            t, tri, bary, hit = md.host_ray_cast(v, f, o, d, t_min, t_max)
            assert np.array_equal(hit, tri >= 0) and np.array_equal(hit, np.isfinite(t)) and np.array_equal(hit, ~np.isnan(bary).any(1))
            assert ((t[hit] >= t_min) & (t[hit] <= t_max)).all()
            t2, bary2, ok = md.host_ray_triangle(v, f, o, d, tri)
            assert np.array_equal(ok, hit) and np.array_equal(t2, t) and np.array_equal(bary2, bary, equal_nan=True), (name, sname)
            assert np.array_equal(md.host_ray_cast(v, f, o, d, t_min, t_max, any_hit=True)[3], hit), (name, sname)
            if name == 'degenerate triangles':
                assert (tri[hit] >= rc.N_REPEATED).all(), sname
                for k in (0, 59, 60, 89):      # ... although they lie exactly on faces that are hit
                    assert not md.host_ray_triangle(v, f, o, d, np.full(len(o), k, dtype=np.int64))[2].any()
            if sname.startswith('NaN'):
                broken = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1))
                assert broken.sum() >= 5 * (len(o) // 8) and not hit[broken].any()


def _view(H, W, fx=100.0, distance=4.0):
    """A camera on the +z axis at ``distance``, looking at the origin: x to the right, y down, z forward (the dataset's OpenCV pose)."""
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0] = K[1, 1] = fx
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[1, 1] = c2w[2, 2] = -1.0
    c2w[2, 3] = distance
    return K[None], c2w[None]


def test_render_view_on_the_host_path():
    """The icosphere(3) seen from (0, 0, 4) at 64 x 64: inside the cone of the inscribed sphere every ray hits, outside the cone of the
    unit sphere none does; only pixels whose ray passes at a distance in [r_in, 1] from the centre are undecided -- at this size
    a ring about 25.8 x (1 - r_in) ~ 0.1 pixel wide around a silhouette of radius 25.8 pixels, under 1 % of the image (the cap of
    10 % is asserted on the analytic sphere)."""
    v, f = rc.icosphere(3)
    r_in = rc.inner_radius(v, f)
    H = W = 64
    K, c2w = _view(H, W)
    out = mr.render_view((v, f), K, c2w, H, W)
    assert all(not x.is_cuda for x in out.values()) and out['mask'].shape == (H, W) and out['normals'].shape == (H, W, 3)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    d = np.stack([(xs - K[0, 0, 2].item()) / 100.0, -(ys - K[0, 1, 2].item()) / 100.0, -np.ones_like(xs, dtype=np.float64)], axis=-1)
    o = np.array([0.0, 0.0, 4.0])
    dist = np.linalg.norm(np.cross(np.broadcast_to(o, d.shape), d), axis=-1) / np.linalg.norm(d, axis=-1)
    undecided = (dist >= r_in) & (dist <= 1.0)
    share = undecided.mean()
    print('r_in = %.6f, undecided pixels: %d of %d (%.2f %%)' % (r_in, undecided.sum(), H * W, 100 * share))
    assert share < 0.10
    mask = out['mask'].numpy()
    assert np.array_equal(mask[~undecided], (dist < 1.0)[~undecided])
    assert 1500 < mask.sum() < 2500                 # pi 25.8^2 = 2091
    t, depth, nrm, pts = out['t'].numpy(), out['depth'].numpy(), out['normals'].numpy(), out['points'].numpy()
    assert np.abs(depth - t * np.linalg.norm(d, axis=-1)).max() <= 4 * 2.0 ** -50       # (values below 8: a few ulps for the norm's roundings)
    assert np.abs(np.linalg.norm(nrm[mask], axis=-1) - 1.0).max() <= 1e-14 and ((nrm[mask] * d[mask]).sum(-1) < 0).all()
    assert np.abs(pts[mask] - (o + t[mask][:, None] * d[mask])).max() <= 1e-15 * 8
    r = np.linalg.norm(pts[mask], axis=-1)
    assert r.min() >= r_in - 1e-12 and r.max() <= 1.0 + 1e-12 and (depth[mask] > 3.0 - 1e-12).all() and (depth[mask] < 4.0).all()
    # on a convex body around the origin the outward face normal is within acos(r_in) of the direction of the point
    assert ((nrm[mask] * pts[mask]).sum(-1) / r >= r_in - 1e-12).all()
    # misses are zeros, as shape_extract leaves them
    assert not t[~mask].any() and not depth[~mask].any() and not nrm[~mask].any() and not pts[~mask].any() and (out['tri'].numpy()[~mask] == -1).all()
    # vertex normals (here the vertices themselves: the sphere's normals) are interpolated, normalised and face the camera
    out_v = mr.render_view((v, f), K, c2w, H, W, vertex_normals=v)
    nv = out_v['normals'].numpy()
    assert np.array_equal(out_v['mask'].numpy(), mask) and np.abs(np.linalg.norm(nv[mask], axis=-1) - 1.0).max() <= 1e-14
    assert ((nv[mask] * pts[mask]).sum(-1) / r >= r_in - 1e-12).all() and not nv[~mask].any()
    # the pixel list in any order gives the same values: render_mesh on the row-major list
    px = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], axis=1)).to(torch.float64)[None]
    flat = mr.render_mesh((v, f), px, K, c2w, scale_mat=torch.eye(4)[None])
    assert torch.equal(flat['t'].reshape(H, W), out['t']) and torch.equal(flat['normals'].reshape(H, W, 3), out['normals'])


def test_mesh_light_visibility_on_the_host_path():
    """Two objects: a floor z = 0 over [-4, 4]^2 that carries the points, and a plate z = 1 over [-1, 1]^2 above it.  A light is hidden
    from a point exactly when its direction rises (l_z > 0) and the shadow ray meets the plate between lnear and lfar; the floor
    itself never hides a light (its rays start on it, below lnear, or run inside its plane)."""
    def square(z, h):
        return np.array([[-h, -h, z], [h, -h, z], [h, h, z], [-h, h, z]], dtype=np.float64)
    v = np.concatenate([square(0.0, 4.0), square(1.0, 1.0)])
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    g = np.random.RandomState(2)
    pts = np.concatenate([(g.random_sample((60, 2)) - 0.5) * 4.0, np.zeros((60, 1))], axis=1)
    lights = np.array([[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0], [0.6, 0.0, 0.8], [-0.5, 0.5, 0.5], [0.3, -0.4, -0.2], [0.0, 0.95, 0.05]])
    vis = mr.mesh_light_visibility((v, f), pts, lights)
    assert vis.shape == (7, 60) and vis.dtype == torch.bool and not vis.is_cuda
    unit = lights / np.linalg.norm(lights, axis=1, keepdims=True)
    rising = unit[:, 2] > 0
    t = np.where(rising, 1.0 / np.where(rising, unit[:, 2], 1.0), np.inf)[:, None]      # [L, 1]: where the ray reaches z = 1
    at = pts[None, :, :2] + np.where(rising[:, None], t, 0.0)[:, :, None] * unit[:, None, :2]
    assert np.abs(np.abs(at[rising]) - 1.0).min() > 1e-6                         # (no ray grazes the plate's rim)
    hidden = rising[:, None] & (t >= 0.1) & (t <= 3.5) & (np.abs(at) < 1.0).all(-1)
    assert hidden.sum() >= 20 and hidden.any(axis=1).sum() >= 3      # (both outcomes occur, under several lights)
    assert np.array_equal(vis.numpy(), ~hidden)
    # the window: with lfar below the plate nothing is hidden, and the layout is [L, Ns] for a single light too
    assert mr.mesh_light_visibility((v, f), pts, lights, lfar=0.9).all()
    assert mr.mesh_light_visibility((v, f), pts, lights[:1]).shape == (1, 60)


def test_render_mesh_tool_on_the_host_path(tmp_path):
    """tools/render_mesh.py --host on the icosphere(2) written as .ply, one view from a params.json: the maps are written, the
    ground-truth comparison runs (against p / |p| at the rendered point p the face normal is within acos(r_in) on a convex body
    around the origin), and of two lights along the viewing axis the one behind the camera is visible from every surface pixel and
    the one behind the sphere from none."""
    import json
    from psnerf_amd.stage1.extracting import Mesh
    from tools import render_mesh
    v, f = rc.icosphere(2)
    r_in = rc.inner_radius(v, f)
    H, W = 48, 64
    K, c2w = _view(H, W)
    Mesh(v, f).export(str(tmp_path / 'mesh.ply'))
    gl = c2w[0].numpy().copy()
    gl[:3, 1:3] *= -1.0                                        # the file holds OpenGL poses
    with open(tmp_path / 'params.json', 'w') as fh:
        json.dump({'K': K[0, :3, :3].tolist(), 'pose_c2w': [gl.tolist()], 'imhw': [H, W], 'n_view': 1, 'gt_normal_world': True}, fh)
    with open(tmp_path / 'lights.json', 'w') as fh:
        json.dump([[0.0, 0.0, 1.0], [0.0, 0.0, -2.0]], fh)
    out = tmp_path / 'maps'
    common = ['--mesh', str(tmp_path / 'mesh.ply'), '--cameras', str(tmp_path / 'params.json'), '--out', str(out), '--host']
    render_mesh.main(common + ['--lights', str(tmp_path / 'lights.json')])
    mask, depth, normal = (np.load(out / sub / 'view_01.npy') for sub in ('mask', 'depth', 'normal'))
    assert mask.shape == (H, W) and mask.dtype == np.bool_ and depth.dtype == np.float32 and normal.shape == (H, W, 3)
    ref = mr.render_view(md.load_mesh(str(tmp_path / 'mesh.ply')), K.float(), c2w.float(), H, W)      # (the file rounds the vertices)
    assert np.array_equal(mask, ref['mask'].numpy()) and np.array_equal(depth, ref['depth'].float().numpy()) and 500 < mask.sum() < H * W
    shadow = np.load(out / 'shadow' / 'view_01.npy')
    assert shadow.shape == (2, H, W) and shadow[0].all() and not shadow[1][mask].any() and shadow[1][~mask].all()
    # the ground truth p / |p| at the rendered points
    gt = ref['points'].numpy() / np.maximum(np.linalg.norm(ref['points'].numpy(), axis=-1, keepdims=True), 1e-30)
    (tmp_path / 'gt').mkdir()
    np.save(tmp_path / 'gt' / 'view_01.npy', gt.astype(np.float32))
    maes = render_mesh.main(common + ['--gt-normal', str(tmp_path / 'gt'), '--views', '1'])
    assert len(maes) == 1 and 0.0 < maes[0] <= np.degrees(np.arccos(r_in))
