"""The definition of the view projection (psnerf_amd/meshproject.py:host_project_rows) and the layers built on it, on the host:
closed forms on a convex mesh, rows blocked by construction, an affine image, the round trip through meshrender with a bound the test
derives, the rules at their edges, bake_views, evaluate_mesh(visible_from=) and trim_unseen."""
import types

import numpy as np
import pytest
import torch

from tests import bake_cases as bc, hull_cases as hc, occlusion_cases as oc, project_cases as pc, raycast_cases as rc
from psnerf_amd import hull
from psnerf_amd import meshbake as mb
from psnerf_amd import meshdist as md
from psnerf_amd import meshproject as mp
from psnerf_amd import meshtopo
from psnerf_amd.meshcore import Mesh

EPS = 2.0 ** -53


def face_rows_of(v, f):
    return mp.face_rows(v, f)


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize('V', [1, 6, 33])
def test_visibility_on_a_convex_mesh_is_the_closed_form(V):
    """Nothing blocks a row of a convex mesh that was lifted off it along its outward normal: seen = in front, in the footprint, facing."""
    v, f = pc.sphere(2)
    _, K, poses = hc.sphere_rig(V)
    H, W = hc.RIG_H, hc.RIG_W
    p, n, _ = oc.surface_rows(v, f, 200, seed=V)
    want = pc.closed_form_convex(p, n, K, poses, H, W)
    img = pc.images(V, H, W, 1, np.uint8, V)
    got = mp.host_project_rows(v, f, p, n, img, K, poses, bias=1e-4, bits=True)
    assert np.array_equal(got.n_seen, want.sum(axis=1))
    assert np.array_equal(mp.unpack_bits(got.words, V), want)
    assert got.words.shape == (200, (V + 31) // 32)
    # best_view: the seeing view of the largest cosine, computed directly
    e = poses[None, :, :3, 3].astype(np.float64) - p[:, None, :]
    c = np.where(want, (n[:, None, :] * e).sum(axis=2) / np.linalg.norm(e, axis=2), -np.inf)
    assert np.array_equal(got.best_view, np.where(want.any(axis=1), c.argmax(axis=1), -1))
    assert 0 < want.sum() < want.size                      # (the ring is in the plane z = 0: rows at the poles face no camera)
    # the same without images: the integers and the weight agree, the sums are absent
    bare = mp.host_project_rows(v, f, p, n, None, K, poses, bias=1e-4, bits=True, hw=(H, W))
    assert bare.sum is None and bare.sum_sq is None and bare.best_value is None
    for key in ('weight', 'n_seen', 'best_view', 'words'):
        assert np.array_equal(getattr(bare, key), getattr(got, key)), key


def test_rows_blocked_by_construction():
    """corner_mesh: a floor z = 0 and a wall x = 0.  A floor row at x = -10 with a camera at x = +30: the segment crosses the wall, so the
    view does not see it; a camera on the row's own side does.  Both face the row and hold it in their image."""
    v, f = oc.corner_mesh()
    p, n = np.array([[-10.0, 0.0, 0.0]]), np.array([[0.0, 0.0, 1.0]])
    H, W = 48, 64
    K = hc.intrinsics(40.0, H, W)
    poses = np.stack([hc.look_at((30.0, 0.0, 20.0), (-10.0, 0.0, 0.0)), hc.look_at((-40.0, 0.0, 20.0), (-10.0, 0.0, 0.0))])
    seg = md.host_ray_cast(v, f, p + 1e-3 * n, poses[0, :3, 3].astype(np.float64)[None] - (p + 1e-3 * n), 0.0, 1.0)
    assert seg[3][0] and seg[1][0] in (2, 3)                                   # the wall's triangles are the ones crossed
    got = mp.host_project_rows(v, f, p, n, None, K, poses, bias=1e-3, bits=True, hw=(H, W))
    assert got.n_seen[0] == 1 and got.best_view[0] == 1 and got.words[0, 0] == 2
    assert pc.closed_form_convex(p, n, K, poses, H, W).all()                   # (only the wall keeps view 0 from it)
    # the sphere behind the rod of the marching-cubes mesh: a point of the sphere below the rod, a camera straight above the rod
    mv, mf = rc.mc_mesh()
    above = hc.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    rows_p, rows_n, _ = oc.surface_rows(mv, mf, 400, seed=3)
    res = mp.host_project_rows(mv, mf, rows_p, rows_n, None, hc.intrinsics(60.0, 64, 64), above[None], hw=(64, 64), bias=1e-4)
    plain = pc.closed_form_convex(rows_p, rows_n, hc.intrinsics(60.0, 64, 64), above[None], 64, 64)[:, 0]
    assert (res.n_seen[~plain] == 0).all() and 0 < (res.n_seen[plain] == 0).sum() < plain.sum()     # some facing rows are in a shadow


def test_an_affine_image_is_reproduced():
    """Float32 images a(x, y) = alpha + beta x + gamma y with small dyadic coefficients hold every pixel exactly, and the bilinear rule
    reproduces an affine function: val = alpha + beta u + gamma v up to four products and three sums of one rounding each on values
    bounded by max |a|, and the expectation's own rounding: 16 x 2^-53 x max |a|."""
    v, f = pc.sphere(2)
    V = 6
    _, K, poses = hc.sphere_rig(V)
    H, W = hc.RIG_H, hc.RIG_W
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    coeff = np.array([[0.5, 0.125, -0.25], [-1.0, 0.03125, 0.0625], [2.0, -0.5, 0.25]])                 # [C, (alpha, beta, gamma)]
    img64 = coeff[:, 0] + coeff[:, 1] * xs[..., None] + coeff[:, 2] * ys[..., None]
    img = np.repeat(img64.astype(np.float32)[None], V, axis=0)
    assert np.array_equal(img[0].astype(np.float64), img64)
    bound = 16.0 * EPS * np.abs(img64).max()
    p, n, _ = oc.surface_rows(v, f, 150, seed=1)
    table = hull._views(K, poses)
    checked = 0
    for view in range(V):
        got = mp.host_project_rows(v, f, p, n, img[view:view + 1], K, poses[view:view + 1], bias=1e-4)
        pu, pv, _ = hull._project_uv(p, table[view])
        seen = got.n_seen == 1
        want = coeff[:, 0] + coeff[:, 1] * pu[seen, None] + coeff[:, 2] * pv[seen, None]
        assert np.abs(got.best_value[seen] - want).max() <= bound
        checked += int(seen.sum())
    assert checked > 150


def test_round_trip_through_the_renderer():
    """Render the mesh from each camera, colour each hit by a world-affine field f, take the silhouettes as masks and project back onto
    the vertices.  A sample is a convex combination of its four footprint pixels, each f at that pixel's hit point stored as float32,
    so for every seen (row, view) and channel |val - f(p)| <= |grad f| max_k |hit_k - p| + 2^-24 max |f| (the storage) + 16 x 2^-53
    max |f| (the bilinear rule's own rounding, as in the affine test).  The bound is computed here from the render's points map."""
    from psnerf_amd import meshrender
    v, f = pc.sphere(2)
    V = 4
    _, K, poses = hc.sphere_rig(V)
    H, W = hc.RIG_H, hc.RIG_W
    A, B = bc.AFFINE_A[:3], bc.AFFINE_B[:3]
    field = lambda x: x @ A.T + B
    imgs, masks, hits = [], [], []
    for view in range(V):
        r = meshrender.render_view((v, f), torch.from_numpy(K.copy())[None], torch.from_numpy(poses[view].copy())[None], H, W)
        hit, pts = r['mask'].numpy(), r['points'].numpy()
        imgs.append(np.where(hit[..., None], field(pts), 0.0).astype(np.float32))
        masks.append(hit)
        hits.append(pts)
    imgs, masks = np.stack(imgs), np.stack(masks)
    vn = meshtopo.vertex_normals((v, f))
    table = hull._views(K, poses)
    f_max = np.abs(field(v)).max() * 1.01
    grad = np.linalg.norm(A, axis=1)
    checked, worst = 0, 0.0
    for view in range(V):
        got = mp.vertex_views((v, f), imgs[view:view + 1], K, poses[view:view + 1], masks=masks[view:view + 1])
        seen = np.nonzero(got.n_seen == 1)[0]
        pu, pv, _ = hull._project_uv(v[seen], table[view])
        x0, y0 = np.floor(pu).astype(int), np.floor(pv).astype(int)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        assert masks[view][y0, x0].all() and masks[view][y1, x1].all()
        far = np.max([np.linalg.norm(hits[view][yy, xx] - v[seen], axis=1) for yy in (y0, y1) for xx in (x0, x1)], axis=0)
        bound = grad[None, :] * far[:, None] + (2.0 ** -24 + 16.0 * EPS) * f_max
        err = np.abs(got.best_value[seen] - field(v[seen]))
        assert (err <= bound).all(), (err - bound).max()
        checked += len(seen)
        worst = max(worst, float((err / bound).max()))
    print('round trip: %d seen (vertex, view) pairs, the worst error is %.3f of its bound' % (checked, worst))
    assert checked > 100


# ------------------------------------------------------------------------------------------------ the rules at their edges
def far_triangle():
    """One triangle far behind everything the edge tests look at: a mesh that blocks nothing."""
    return np.array([[100.0, 100.0, 50.0], [101.0, 100.0, 50.0], [100.0, 101.0, 50.0]]), np.array([[0, 1, 2]], dtype=np.int64)


def axis_view(H, W):
    K, c2w = hc.axis_camera(H, W)                    # at (0, 0, -2) looking along +z, fx = 64, principal point (16, 8): exact products
    return K, c2w[None]


def at(u, v):
    return [(u - 16.0) / 64.0 * 2.0, (v - 8.0) / 64.0 * 2.0, 0.0]


def test_footprint_edges():
    H, W = 17, 33
    mv, mf = far_triangle()
    K, pose = axis_view(H, W)
    eps = 2.0 ** -20
    pts = np.array([at(0.0, 3.0), at(-eps, 3.0), at(W - 1.0, 3.0), at(W - 1.0 + eps, 3.0), at(5.0, 0.0), at(5.0, -eps), at(5.0, H - 1.0),
                    at(5.0, H - 1.0 + eps), [0.0, 0.0, -3.0], [0.0, 0.0, -2.0]])
    n = np.tile([0.0, 0.0, -1.0], (len(pts), 1))
    img = pc.images(1, H, W, 3, np.float32)
    got = mp.host_project_rows(mv, mf, pts, n, img, K, pose, bias=0.0)
    assert got.n_seen.tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 0, 0]                       # (the last two: behind the camera, and at its centre)
    wide = img[0].astype(np.float64)
    assert np.array_equal(got.best_value[0], wide[3, 0]) and np.array_equal(got.best_value[2], wide[3, W - 1])     # x1 = x0 = W - 1, fx = 0
    assert np.array_equal(got.best_value[4], wide[0, 5]) and np.array_equal(got.best_value[6], wide[H - 1, 5])


@pytest.mark.parametrize('hw', [(1, 1), (1, 9), (9, 1)])
def test_images_of_one_row_or_column(hw):
    H, W = hw
    mv, mf = far_triangle()
    K = np.array([[64.0, 0.0, 0.0], [0.0, 64.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    pose = np.eye(4, dtype=np.float32)[None]
    pose[0, 2, 3] = -2.0
    img = pc.images(1, H, W, 4, np.uint8, seed=H + W)
    pts = np.array([[0.0, 0.0, 0.0], [2.5 / 32.0 if W > 1 else 0.0, 2.5 / 32.0 if H > 1 else 0.0, 0.0]])     # (u, v) = (0, 0) and 2.5 where there is room
    got = mp.host_project_rows(mv, mf, pts, np.tile([0.0, 0.0, -1.0], (2, 1)), img, K, pose, bias=0.0)
    assert got.n_seen.tolist() == [1, 1]
    wide = img[0].astype(np.float64) / 255.0
    assert np.array_equal(got.best_value[0], wide[0, 0])
    x0, y0 = (2 if W > 1 else 0), (2 if H > 1 else 0)
    x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
    fx, fy = (0.5 if W > 1 else 0.0), (0.5 if H > 1 else 0.0)
    want = (1.0 - fy) * ((1.0 - fx) * wide[y0, x0] + fx * wide[y0, x1]) + fy * ((1.0 - fx) * wide[y1, x0] + fx * wide[y1, x1])
    assert np.array_equal(got.best_value[1], want)


def test_facing_is_strict():
    mv, mf = far_triangle()
    K, pose = axis_view(17, 33)
    p, n = np.array([[0.0, 0.0, 0.0]]), np.array([[0.0, 0.0, -1.0]])                    # e = (0, 0, -2): c = 2 / 2 = 1 exactly
    for cos_min, seen in ((1.0, 0), (np.nextafter(1.0, 0.0), 1), (0.0, 1)):
        assert mp.host_project_rows(mv, mf, p, n, None, K, pose, bias=0.0, cos_min=cos_min, hw=(17, 33)).n_seen[0] == seen
    away = mp.host_project_rows(mv, mf, p, -n, None, K, pose, bias=0.0, hw=(17, 33))
    assert away.n_seen[0] == 0 and mp.host_project_rows(mv, mf, p, -n, None, K, pose, bias=0.0, cos_min=-1.5, hw=(17, 33)).n_seen[0] == 1


def test_mask_needs_all_four_pixels():
    H, W = 17, 33
    mv, mf = far_triangle()
    K, pose = axis_view(H, W)
    p, n = np.array([at(5.5, 3.5)]), np.array([[0.0, 0.0, -1.0]])
    full = np.ones((1, H, W), dtype=np.uint8)
    assert mp.host_project_rows(mv, mf, p, n, None, K, pose, masks=full, bias=0.0, hw=(H, W)).n_seen[0] == 1
    for y, x in ((3, 5), (3, 6), (4, 5), (4, 6)):
        m = full.copy()
        m[0, y, x] = 0
        assert mp.host_project_rows(mv, mf, p, n, None, K, pose, masks=m, bias=0.0, hw=(H, W)).n_seen[0] == 0, (y, x)
    for y, x in ((2, 5), (5, 6), (3, 4), (4, 7)):                                       # the ring around the footprint does not matter
        m = full.copy()
        m[0, y, x] = 0
        assert mp.host_project_rows(mv, mf, p, n, None, K, pose, masks=m * 7, bias=0.0, hw=(H, W)).n_seen[0] == 1, (y, x)
    on_pixel = mp.host_project_rows(mv, mf, np.array([at(5.0, 3.0)]), n, None, K, pose, masks=full * (np.arange(W) != 6)[None, None, :], bias=0.0,
                                    hw=(H, W))
    assert on_pixel.n_seen[0] == 0                                                      # fx = 0 still reads x1 = x0 + 1: the rule, not the weight


def test_ties_weights_and_channels():
    v, f = pc.sphere(2)
    _, K, poses = hc.sphere_rig(6)
    H, W = hc.RIG_H, hc.RIG_W
    p, n, _ = oc.surface_rows(v, f, 120, seed=5)
    for C in (1, 3, 4):
        img = pc.images(6, H, W, C, np.float32 if C != 3 else np.uint8, seed=C)
        twice = mp.host_project_rows(v, f, p, n, img[[2, 2]], K, poses[[2, 2]], bias=1e-4)
        once = mp.host_project_rows(v, f, p, n, img[[2]], K, poses[[2]], bias=1e-4)
        seen = once.n_seen == 1
        assert seen.any() and np.array_equal(twice.n_seen, 2 * once.n_seen) and (twice.best_view[seen] == 0).all()       # a tie: the lower view
        assert np.array_equal(twice.sum, once.sum + once.sum) and np.array_equal(twice.best_value, once.best_value)
        assert once.sum.shape == (120, C)
        cosine = mp.host_project_rows(v, f, p, n, img, K, poses, bias=1e-4)
        uniform = mp.host_project_rows(v, f, p, n, img, K, poses, bias=1e-4, weight='uniform')
        assert np.array_equal(uniform.n_seen, cosine.n_seen) and np.array_equal(uniform.weight, cosine.n_seen.astype(np.float64))
        assert (cosine.weight[cosine.n_seen > 0] < cosine.n_seen[cosine.n_seen > 0]).all()
        lowest = np.array([np.nonzero(r)[0][0] if r.any() else -1 for r in pc.closed_form_convex(p, n, K, poses, H, W)])
        assert np.array_equal(uniform.best_view, lowest)                               # all weights equal: the lowest seeing view
        # the helpers: mean, spread and the single-view identities
        m, s = mp.mean(cosine), mp.spread(cosine)
        assert (m[cosine.n_seen == 0] == 0).all() and (s >= 0).all() and np.isfinite(m).all() and np.isfinite(s).all()
        one = mp.host_project_rows(v, f, p, n, img[[2]], K, poses[[2]], bias=1e-4, weight='uniform')
        assert np.array_equal(mp.mean(one)[seen], one.best_value[seen]) and np.abs(mp.spread(one)).max() <= 1e-7


def test_camera_normals_are_the_trainers_rotation():
    """frame='camera_normal' against stage1.training.Trainer._targets_torch: the raw sample of a view, handed to the trainer's own
    rotation as a constant normal map in float64, comes back as the camera_normal sample, bit for bit."""
    from psnerf_amd.stage1.training import Trainer
    v, f = pc.sphere(2)
    K, poses = pc.cameras(v, 5, 40, 32, seed=2)
    img = pc.images(5, 40, 32, 3, np.float32, seed=9)
    p, n, _ = oc.surface_rows(v, f, 60, seed=2)
    stub = types.SimpleNamespace(normal_loss=False, angle=None)
    checked = 0
    for view in range(5):
        raw = mp.host_project_rows(v, f, p, n, img[[view]], K, poses[[view]], bias=1e-4)
        world = mp.host_project_rows(v, f, p, n, img[[view]], K, poses[[view]], bias=1e-4, frame='camera_normal')
        assert np.array_equal(raw.n_seen, world.n_seen)
        for row in np.nonzero(raw.n_seen)[0][:6]:
            normal = torch.from_numpy(raw.best_value[row].copy()).reshape(1, 3, 1, 1).expand(1, 3, 2, 2).contiguous()
            ones = torch.ones(1, 1, 2, 2, dtype=torch.float64)
            got = Trainer._targets_torch(stub, ones.expand(1, 3, 2, 2), ones, ones, normal, ones, torch.from_numpy(poses[view].astype(np.float64))[None],
                                         torch.zeros(1, 1, 2, dtype=torch.float64), True)[4]
            assert np.array_equal(got.numpy().reshape(3), world.best_value[row])
            checked += 1
    assert checked >= 12
    fused = mp.fused_normals(world)
    length = np.linalg.norm(fused, axis=1)
    assert np.allclose(length[world.n_seen > 0], 1.0) and (length[world.n_seen == 0] == 0).all()
    with pytest.raises(ValueError, match='camera_normal'):
        mp.host_project_rows(v, f, p, n, img[..., :1], K, poses, frame='camera_normal')


def test_degenerate_rows_and_arguments():
    v, f = pc.sphere(2)
    _, K, poses = hc.sphere_rig(6)
    H, W = hc.RIG_H, hc.RIG_W
    p, n, _ = oc.surface_rows(v, f, 40, seed=8)
    p, n, dead = oc.degenerate_rows(p, n)
    img = pc.images(6, H, W, 3, np.uint8)
    got = mp.host_project_rows(v, f, p, n, img, K, poses, bits=True)
    assert dead.sum() == 5 and (got.n_seen[dead] == 0).all() and (got.best_view[dead] == -1).all() and (got.words[dead] == 0).all()
    assert (got.sum[dead] == 0).all() and (got.sum_sq[dead] == 0).all() and (got.weight[dead] == 0).all() and (got.best_value[dead] == 0).all()
    assert got.n_seen[~dead].sum() > 0 and got.n_seen.dtype == np.int32 and got.best_view.dtype == np.int32 and got.words.dtype == np.int32
    unseen = got.n_seen == 0
    assert (got.best_view[unseen] == -1).all() and (got.best_value[unseen] == 0).all()
    for bad in (dict(weight='area'), dict(frame='world'), dict(bias=np.inf), dict(cos_min=np.nan)):
        with pytest.raises(ValueError):
            mp.host_project_rows(v, f, p, n, img, K, poses, **bad)
    for images in (img[:5], img.astype(np.float64), np.zeros((6, H, W, 5), dtype=np.uint8), img[0]):
        with pytest.raises(ValueError):
            mp.host_project_rows(v, f, p, n, images, K, poses)
    with pytest.raises(ValueError):
        mp.host_project_rows(v, f, p, n, None, K, poses)                                # no images and no hw
    with pytest.raises(ValueError):
        mp.host_project_rows(v, f, p, n, img, K, poses, masks=np.ones((6, H, W + 1), dtype=np.uint8))
    with pytest.raises(RuntimeError, match='CPU tensors'):
        mp.project_rows((torch.from_numpy(v.copy()), torch.from_numpy(f.copy())), p, n, img, K, poses)


def test_hull_projection_is_one_statement():
    """hull._project is hull._project_uv rounded: host_project (and with it the carving) returns what it did."""
    K, pose = hc.random_camera(3, 48, 64)
    pts = np.random.RandomState(0).randn(500, 3)
    table = hull._views(K, pose)
    pu, pv, front = hull._project_uv(pts, table[0])
    fu, fv, front2 = hull._project(pts, table[0])
    assert np.array_equal(fu, np.floor(pu + 0.5)) and np.array_equal(fv, np.floor(pv + 0.5)) and np.array_equal(front, front2)
    ix, iy, inside = hull.host_project(pts, K, pose, (48, 64))
    want = front & (fu >= 0) & (fu < 64) & (fv >= 0) & (fv < 48)
    assert np.array_equal(inside, want) and np.array_equal(ix[inside], fu[inside].astype(np.int64)) and inside.any()


# ------------------------------------------------------------------------------------------------ the layers
@pytest.mark.parametrize('name', ['icosphere(1)', 'a tetrahedron', 'zero-area faces'])
def test_bake_views_in_chunks_equals_one_call(name):
    v, f, vn = bc.meshes()[name]
    mesh = (v, f) if vn is None else (v, f, vn)
    H, W = 40, 32
    K, poses = pc.cameras(v, 5, H, W, seed=1)
    img = pc.images(5, H, W, 3, np.uint8, seed=4)
    one = mb.bake_views(mesh, img, K, poses, size=64, fill=0.25)
    parts = mb.bake_views(mesh, img, K, poses, atlas=one['atlas'], fill=0.25, chunk_faces=max(1, len(f) // 3))
    assert set(one) == {'atlas', 'photo', 'photo_best', 'seen', 'spread'}
    for key in ('photo', 'photo_best', 'seen', 'spread'):
        assert one[key].dtype == np.float32 and one[key].shape == (64, 64, 1 if key == 'seen' else 3)
        assert np.array_equal(one[key].view(np.uint32), parts[key].view(np.uint32)), key
    owned = one['atlas'].owner()[0] >= 0
    seen = one['seen'][..., 0]
    assert (seen[~owned] == 0.25).all() and (seen[owned] >= 1.0).any() and set(np.unique(seen[owned])) <= {0.25, 1.0, 2.0, 3.0, 4.0, 5.0}
    lit = owned & (seen >= 1.0)
    assert (one['photo'][lit] >= 0.0).all() and (one['photo'][lit] <= 1.0).all() and (one['photo'][owned & (seen == 0.25)] == 0.25).all()


def test_export_textured_with_and_without_the_photo(tmp_path):
    """Without the new keys every file is what it was (the same call on a dict with and without them, the photo files aside); with
    them name_photo.png and name_seen.png appear and the .mtl names them in one comment line more."""
    v, f, vn = bc.meshes()['icosphere(1)']
    H, W = 40, 32
    K, poses = pc.cameras(v, 3, H, W)
    occl = mb.bake_occlusion((v, f, vn), size=64, K=4)
    views = mb.bake_views((v, f, vn), pc.images(3, H, W, 3, np.uint8), K, poses, atlas=occl['atlas'])
    before = mb.export_textured(str(tmp_path / 'a' / 'm.obj'), (v, f, vn), occl)
    after = mb.export_textured(str(tmp_path / 'b' / 'm.obj'), (v, f, vn), dict(occl, **views))
    assert set(after) - set(before) == {'photo', 'seen'} and 'photo' not in before
    read = lambda path: open(path, 'rb').read()
    for key in before:
        if key != 'mtl':
            assert read(before[key]) == read(after[key]), key
    old, new = read(before['mtl']).decode().splitlines(), read(after['mtl']).decode().splitlines()
    assert new[:len(old)] == old and len(new) == len(old) + 1 and new[-1].startswith('#') and 'm_photo.png' in new[-1] and 'm_seen.png' in new[-1]
    from PIL import Image
    assert np.asarray(Image.open(after['photo'])).shape == (64, 64, 3) and np.asarray(Image.open(after['seen'])).max() in (1, 2, 3)


def one_sided(V=5):
    """Cameras on a third of the ring of hull_cases.sphere_rig(12): they see one side of the sphere only."""
    _, K, poses = hc.sphere_rig(12)
    return K, poses[:V]


def test_evaluate_mesh_visible_from():
    from psnerf_amd.mesheval import evaluate_mesh
    pred, gt = Mesh(*pc.sphere(2)), Mesh(*pc.sphere(3))
    K, poses = one_sided()
    H, W = hc.RIG_H, hc.RIG_W
    plain = evaluate_mesh(pred, gt, 1500, iou_points=2000, rng=np.random.RandomState(3))
    again = evaluate_mesh(pred, gt, 1500, iou_points=2000, rng=np.random.RandomState(3), visible_from=None)
    assert set(plain) == set(again) and all(np.array_equal(plain[k], again[k]) for k in plain if k != 'raw')
    assert all(np.array_equal(plain['raw'][k], again['raw'][k]) for k in plain['raw']) and 'visible_fraction_pred' not in plain
    seen = evaluate_mesh(pred, gt, 1500, iou_points=2000, rng=np.random.RandomState(3), visible_from=(K, poses, H, W))
    for side, mesh in (('pred', pred), ('gt', gt)):
        pts, face = seen['raw'][side + '_surf_pts'], seen['raw'][side + '_face']
        assert np.array_equal(pts, plain['raw'][side + '_surf_pts'])                    # the samples are drawn exactly as without
        normals = oc.geometric_normals(mesh.vertices, mesh.faces, face)
        keep = pc.closed_form_convex(pts, normals, K, poses, H, W).any(axis=1)
        assert np.array_equal(seen['raw'][side + '_visible'], keep)
        assert 0.0 < seen['visible_fraction_' + side] == keep.mean() < 1.0
    kd = plain['raw']['pred_gt_dist'][seen['raw']['pred_visible']]
    assert seen['accuracy'] == float(kd.mean()) and seen['accuracy2'] == float((kd * kd).mean())
    kc = plain['raw']['gt_pred_dist'][seen['raw']['gt_visible']]
    assert seen['completeness'] == float(kc.mean()) and seen['chamfer'] == float((kd.mean() + kc.mean()) / 2)
    t = seen['thresholds'][1]
    assert seen['precision_count'][t] == int((kd <= t).sum()) and seen['recall'][t] == int((kc <= t).sum()) / len(kc)
    for key in ('iou', 'inside_pred', 'inside_gt', 'union', 'thresholds'):
        assert seen[key] == plain[key], key
    with pytest.raises(ValueError, match='no sample'):
        away = hc.look_at((0.0, 5.0, 0.0), (0.0, 10.0, 0.0))[None]
        evaluate_mesh(pred, gt, 50, iou_points=0, rng=np.random.RandomState(3), visible_from=(K, away, H, W))


def test_trim_unseen_and_face_visibility():
    v, f = pc.sphere(2)
    K, poses = one_sided()
    H, W = hc.RIG_H, hc.RIG_W
    centroid, normal = face_rows_of(v, f)
    assert np.allclose(centroid, v[f].mean(axis=1)) and np.allclose(normal, oc.geometric_normals(v, f, np.arange(len(f))))
    want = pc.closed_form_convex(centroid, normal, K, poses, H, W)
    n_seen = mp.face_visibility((v, f), K, poses, H, W)
    assert np.array_equal(n_seen, want.sum(axis=1)) and n_seen.dtype == np.int32
    whole = mp.face_visibility((v, f), K, poses, H, W, result=True, bits=True)
    assert np.array_equal(mp.unpack_bits(whole.words, len(poses)), want) and whole.sum is None
    keep = want.any(axis=1)
    assert 0 < keep.sum() < len(f)
    vn = meshtopo.vertex_normals((v, f))
    trimmed, seen = mp.trim_unseen(Mesh(v, f, vertex_normals=vn), K, poses, H, W)
    assert np.array_equal(seen, n_seen) and trimmed.faces.shape == (int(keep.sum()), 3)
    used = np.unique(f[keep])                                                           # compacted: the used vertices in their order
    assert np.array_equal(trimmed.vertices, v[used]) and np.array_equal(trimmed.vertex_normals, vn[used])
    assert np.array_equal(trimmed.vertices[trimmed.faces], v[f[keep]])
    # a zero-area face has a zero normal and is never seen; masks are honoured
    zv, zf, _ = bc.meshes()['zero-area faces']
    zK, zposes = pc.cameras(zv, 8, H, W)
    z_seen = mp.face_visibility((zv, zf), zK, zposes, H, W)
    assert (z_seen[10:13] == 0).all() and z_seen.sum() > 0
    assert mp.face_visibility((v, f), K, poses, H, W, masks=np.zeros((len(poses), H, W), dtype=np.uint8)).sum() == 0


def test_project_views_tool_on_the_host(tmp_path):
    """tools/project_views.py --host on a hull_cases.write_dataset directory: the files it promises and a report that adds up."""
    import json
    import os
    import subprocess
    import sys
    from PIL import Image
    V = 6
    params, mask_dir = hc.write_dataset(tmp_path / 'obj', V)
    masks, K, poses = hc.sphere_rig(V)
    v, f = pc.sphere(2)
    mesh_path = str(tmp_path / 'mesh.obj')
    Mesh(v, f).export(mesh_path)
    g = np.random.RandomState(0)
    for view in range(V):
        folder = tmp_path / 'obj' / 'img' / ('view_%02d' % (view + 1))
        os.makedirs(str(folder), exist_ok=True)
        for light in (1, 2):
            Image.fromarray((g.randint(0, 256, (hc.RIG_H, hc.RIG_W, 3)) * (masks[view][..., None] > 0)).astype(np.uint8)).save(
                str(folder / ('%03d.png' % light)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / 'out' / 'sphere')
    done = subprocess.run([sys.executable, os.path.join(root, 'tools', 'project_views.py'), mesh_path, str(tmp_path / 'obj'), '--host', '--light', '2',
                           '--size', '64', '--out', out], capture_output=True, text=True, cwd=root)
    assert done.returncode == 0, done.stderr[-2000:]
    report = json.loads(done.stdout.strip().splitlines()[-1])
    assert 0.5 < report['area_seen'] <= 1.0 and report['mean_spread'] >= 0.0 and report['n_views'] == V and report['path'] == 'host'
    for suffix in ('_photo.png', '_seen.png', '_vertex_rgb.npy', '_vertex_seen.npy'):
        assert os.path.exists(out + suffix), suffix
    assert np.load(out + '_vertex_rgb.npy').shape == (len(v), 3) and np.load(out + '_vertex_seen.npy').max() <= V
