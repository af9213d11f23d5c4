"""Silhouette carving, the numpy definition (psnerf_amd/hull.py): dilation against a brute-force loop and scipy, the projection
against the camera it inverts (stage1.rendering.pixel_rays / camera_origin), the carving rule on analytic sphere rigs, the extractor's
``carve=`` on the host path, the hull mesh, and the argument checks of the C entry points (which need no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import hull_cases as hc
from psnerf_amd import hull

SIZES = ((1, 1), (5, 7), (24, 20), (33, 70))


# ------------------------------------------------------------------------------------------------ dilation
@pytest.mark.parametrize('shape', sorted(hc.SHAPES))
@pytest.mark.parametrize('r', hc.RADII)
def test_host_dilate_equals_the_loop_over_the_footprint(shape, r):
    fp = hc.SHAPES[shape](r)
    for H, W in SIZES:
        for name in hc.PATTERNS:
            m = hc.pattern(name, 2, H, W)
            for border in (0, 1):
                got = hull.host_dilate(m, fp, border)
                assert got.dtype == np.uint8 and np.array_equal(got, hc.brute_dilate(m, fp, border)), (shape, r, H, W, name, border)
            assert np.array_equal(hull.host_erode(m, fp), 1 - hc.brute_dilate(m == 0, fp, 1))


@pytest.mark.parametrize('shape', sorted(hc.SHAPES))
def test_a_single_pixel_comes_back_as_the_footprint(shape):
    for r in hc.RADII:
        fp = hc.SHAPES[shape](r)
        m = np.zeros((1, 2 * r + 1, 2 * r + 1), dtype=np.uint8)
        m[0, r, r] = 1
        assert np.array_equal(hull.host_dilate(m, fp)[0].astype(bool), hull.footprint_pixels(fp))
    d = np.arange(-12, 13)
    assert np.array_equal(hull.footprint_pixels(hull.disk_footprint(12)), d[:, None] ** 2 + d[None, :] ** 2 <= 144)
    assert np.array_equal(hull.footprint_pixels(hull.diamond_footprint(3)), np.abs(d[9:16, None]) + np.abs(d[None, 9:16]) <= 3)


def test_footprints_are_checked():
    for bad in ([1, 2], [[1]], [0.0, 1.0, 0.0], [0, -1, 0], [0, 2, 0]):
        with pytest.raises(ValueError):
            hull.check_footprint(np.array(bad))
    with pytest.raises(ValueError):
        hull.disk_footprint(-1)
    with pytest.raises(ValueError):
        hull.host_dilate(np.zeros((1, 2, 2)), hull.disk_footprint(1), border=2)
    with pytest.raises(ValueError):
        hull.host_dilate(np.zeros((2, 2)), hull.disk_footprint(1))


def test_diamond_and_mask_valid_against_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    for H, W in SIZES:
        for name in ('random', 'checker', 'centre', 'corners', 'full'):
            m = hc.pattern(name, 1, H, W)[0] != 0
            for r in (1, 2, 12):
                fp = hull.diamond_footprint(r)
                assert np.array_equal(hull.host_dilate(m[None], fp)[0].astype(bool), ndimage.binary_dilation(m, iterations=r))
                assert np.array_equal(hull.host_erode(m[None], fp)[0].astype(bool), ndimage.binary_erosion(m, iterations=r))
            maskd, maske = ndimage.binary_dilation(m, iterations=2), ndimage.binary_erosion(m, iterations=2)
            valid = hull.mask_valid(m)
            assert valid.dtype == np.bool_ and np.array_equal(valid, ~np.logical_xor(maskd, maske))
    blob = np.zeros((40, 50), dtype=np.uint8)                      # a mask like the dataset's: one blob, 0 / 255
    blob[8:30, 10:41] = 255
    assert np.array_equal(hull.mask_valid(blob), ~np.logical_xor(ndimage.binary_dilation(blob, iterations=2), ndimage.binary_erosion(blob, iterations=2)))
    assert np.array_equal(hull.mask_valid(np.stack([blob, blob]))[1], hull.mask_valid(blob))


# ------------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_host_project_inverts_pixel_rays(seed):
    """For float32 cameras, o + t pixel_rays(px) in float32 comes back as the integer pixel px, for three depths."""
    from psnerf_amd.handoff import arange_pixels
    from psnerf_amd.stage1.rendering import camera_origin, pixel_rays
    H, W = 19, 23
    K, c2w = hc.random_camera(seed, H, W)
    px = arange_pixels(H, W, 'cpu')
    cam, world = torch.from_numpy(K)[None], torch.from_numpy(c2w)[None]
    rays = pixel_rays(px.to(torch.float32), cam, world)
    origin = camera_origin(px.shape[1], world)
    for t in (0.25, 1.0, 3.0):
        p = (origin + np.float32(t) * rays)[0]
        assert p.dtype == torch.float32
        ix, iy, inside = hull.host_project(p.numpy(), K, c2w, hw=(H, W), scale_mat=np.eye(4))
        assert inside.all() and np.array_equal(ix, px[0, :, 0].numpy()) and np.array_equal(iy, px[0, :, 1].numpy())
        ix2, iy2, inside2 = hull.host_project(p.numpy(), K, c2w)
        assert inside2.all() and np.array_equal(ix2, ix) and np.array_equal(iy2, iy)
        smaller = hull.host_project(p.numpy(), K, c2w, hw=(H - 2, W - 3))
        assert np.array_equal(smaller[2], (ix < W - 3) & (iy < H - 2)) and (smaller[0][~smaller[2]] == -1).all()
        back = hull.host_project((origin - np.float32(t) * rays)[0].numpy(), K, c2w, hw=(H, W))
        assert not back[2].any() and (back[0] == -1).all() and (back[1] == -1).all()


def test_host_project_odd_points_and_exact_edges():
    H, W = 16, 32
    K, c2w = hc.axis_camera(H, W)
    ix, iy, inside = hull.host_project(hc.odd_points(c2w), K, c2w, hw=(H, W))
    assert inside.tolist() == [False, False, False, False, True] and (ix[4], iy[4]) == (16, 8)
    p, want = hc.edge_points(H, W)
    ix, iy, inside = hull.host_project(p, K, c2w, hw=(H, W))
    assert np.array_equal(inside, want)
    assert ix[[0, 3]].tolist() == [0, W - 1] and iy[[4, 7]].tolist() == [0, H - 1]
    with pytest.raises(ValueError):
        hull.host_project(np.zeros((3, 2)), K, c2w)
    with pytest.raises(ValueError):
        hull.host_project(np.zeros((3, 3)), K, np.eye(3))


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize('V', [1, 3, 8])
@pytest.mark.parametrize('radius', [1, 2, 12])
def test_no_lattice_point_inside_the_sphere_is_carved(V, radius):
    """A condition, not a tolerance: with the silhouettes dilated by at least a pixel every one of the 1237 lattice points of the 33^3
    lattice that lie inside the sphere is kept, in all nine rigs.  (Radius 0 is not part of it: a point on the sphere's limb projects to
    a pixel whose centre may lie just outside the analytic silhouette.)"""
    axis, p = hc.lattice(33)
    keep, by = hc.sphere_carve(V, radius)
    inside = np.linalg.norm(p, axis=1) <= hc.SPHERE_RADIUS
    assert int(inside.sum()) == 1237 and keep[inside].all()
    assert np.array_equal(keep, by == -1) and by.dtype == np.int32 and by.min() >= -2 and by.max() < V
    assert 0 < int(keep.sum()) < p.shape[0] - int((by == -2).sum())      # (something is carved by a view, something is kept)


@pytest.mark.parametrize('V', [1, 3, 8])
def test_carved_by_is_the_lowest_rejecting_view_and_minus_two_where_no_image_sees(V):
    masks, K, poses = hc.sphere_rig(V)
    dil = hull.host_dilate(masks, hull.disk_footprint(2))
    axis, p = hc.lattice(33)
    keep, by = hc.sphere_carve(V, 2)
    seen = np.zeros((V, p.shape[0]), dtype=bool)
    rejects = np.zeros((V, p.shape[0]), dtype=bool)
    for v in range(V):
        ix, iy, inside = hull.host_project(p, K, poses[v], hw=dil.shape[1:])
        seen[v] = inside
        rejects[v, inside] = dil[v, iy[inside], ix[inside]] == 0
    assert np.array_equal(by == -2, ~seen.any(0)) and (by == -2).any()
    first = np.where(rejects.any(0), rejects.argmax(0), -1)
    assert np.array_equal(by[seen.any(0)], first[seen.any(0)])
    if V == 8:
        assert len(np.unique(by)) == V + 2                           # (every view carves some point first)
    # one view at a time composes to the same keep
    alone = [hull.host_carve_points(p, dil[v:v + 1], K, poses[v:v + 1])[1] for v in range(V)]
    assert np.array_equal(keep, seen.any(0) & np.all([a != 0 for a in alone], axis=0))
    # float32 points are widened exactly
    p32 = p.astype(np.float32)
    assert np.array_equal(hull.host_carve_points(p32, dil, K, poses)[1], hull.host_carve_points(p32.astype(np.float64), dil, K, poses)[1])


def test_host_carve_grid_writes_only_the_carved_elements():
    masks, K, poses = hc.sphere_rig(3)
    dil = hull.host_dilate(masks, hull.disk_footprint(2))
    n = 17
    axis = (hc.BOX_SIZE * torch.linspace(-0.5, 0.5, n))
    grid = np.random.RandomState(0).randn(n, n, n).astype(np.float32)
    grid[3, 4, 5], grid[8, 8, 8] = np.float32(-0.0), np.float32(np.nan)
    before = grid.copy()
    keep, _ = hull.host_carve_points(hull.lattice_points(axis.numpy().astype(np.float64)), dil, K, poses)
    keep = keep.reshape(n, n, n)
    count = hull.carve_grid(grid, axis, dil, K, poses)
    assert count == int((~keep).sum()) and 0 < count < n ** 3
    assert (grid[~keep] == np.float32(-30.0)).all() and np.array_equal(grid[keep].view(np.uint32), before[keep].view(np.uint32))
    assert keep[8, 8, 8] and np.isnan(grid[8, 8, 8])
    for bad in (grid.astype(np.float64), grid[:5], grid[:, :, :5]):
        with pytest.raises(ValueError):
            hull.host_carve_grid(bad, axis, dil, K, poses)
    with pytest.raises(ValueError):
        hull.host_carve_grid(grid, axis[:-1], dil, K, poses)
    with pytest.raises(ValueError):
        hull.host_carve_points(np.zeros((4, 3)), dil, K, poses[:2])


# ------------------------------------------------------------------------------------------------ the extractor, host path
def _hull(V=8, radius=2):
    masks, K, poses = hc.sphere_rig(V)
    return hull.VisualHull(masks, K, poses, footprint=hull.disk_footprint(radius))


@pytest.mark.parametrize('kw', [dict(resolution0=8, upsampling_steps=2), dict(resolution0=33, upsampling_steps=0)], ids=['mise', 'flat'])
def test_extractor_carves_the_dense_grid_on_the_host_path(kw):
    from psnerf_amd.stage1.extracting import Extractor3D
    plain = Extractor3D(hc.SphereModel(0.9), **kw)                  # a sphere that reaches beyond the silhouettes' hull
    mesh0, stats0 = plain.generate_mesh()
    vh = _hull()
    ex = Extractor3D(hc.SphereModel(0.9), carve=vh, **kw)
    mesh, stats = ex.generate_mesh()
    n = 33
    axis = hc.BOX_SIZE * torch.linspace(-0.5, 0.5, n)
    keep = vh.contains(hull.lattice_points(axis.numpy().astype(np.float64))).reshape(n, n, n)
    assert ex.last_grid.shape == (n, n, n) and ex.last_grid.dtype == np.float32
    assert np.array_equal(ex.last_grid[keep].view(np.uint32), plain.last_grid[keep].view(np.uint32))
    assert (ex.last_grid[~keep] == np.float32(-30.0)).all()
    assert stats['n_points_carved'] == int((~keep).sum()) > 0 and stats['time (carve)'] >= 0.0
    assert stats['n_points_evaluated'] == stats0['n_points_evaluated'] and 'n_points_carved' not in stats0
    assert 0 < len(mesh.faces) and np.abs(mesh.vertices[:, 2]).max() < np.abs(mesh0.vertices[:, 2]).max()
    # carve=None: the parent's result, bit for bit (the parent's own tests pin it against the recorded fixtures)
    again, _ = Extractor3D(hc.SphereModel(0.9), carve=None, **kw).generate_mesh()
    assert np.array_equal(again.vertices, mesh0.vertices) and np.array_equal(again.faces, mesh0.faces)
    # with clip: carved first, then clipped
    exc = Extractor3D(hc.SphereModel(0.9), carve=vh, **kw)
    exc.generate_mesh(clip=True)
    below = (axis < -1).numpy()
    assert (exc.last_grid[:, :, below] == np.float32(-30.0)).all() and np.array_equal(exc.last_grid[:, :, ~below], ex.last_grid[:, :, ~below])


def test_mask_loader_still_raises_and_names_carve():
    from psnerf_amd.stage1.extracting import Extractor3D
    with pytest.raises(NotImplementedError, match='carve='):
        Extractor3D(hc.SphereModel(), resolution0=8, upsampling_steps=2).generate_mesh(mask_loader=[{}])
    with pytest.raises(NotImplementedError, match='VisualHull.from_loader'):
        Extractor3D(hc.SphereModel(), resolution0=8, upsampling_steps=2, carve=_hull()).generate_mesh(mask_loader=[{}])


# ------------------------------------------------------------------------------------------------ VisualHull
def test_hull_mesh_contains_the_sphere_and_is_one_component():
    from psnerf_amd import meshclean
    from tests import mesh_fields as mf
    vh = _hull(8, 12)
    mesh = vh.mesh(32, hc.BOX_SIZE)
    assert len(mesh.faces) > 1000 and mf.is_closed_oriented(mesh.faces)
    assert np.linalg.norm(mesh.vertices, axis=1).min() >= hc.SPHERE_RADIUS - hc.BOX_SIZE / 32
    assert np.abs(mesh.vertices).max() < hc.BOX_SIZE / 2                 # the empty outer layer closes the hull inside the box
    labels, table = meshclean.components(mesh.vertices, mesh.faces)
    assert len(table['label']) == 1
    grid, axis = vh.indicator(32, hc.BOX_SIZE)
    assert set(np.unique(grid).tolist()) == {-1.0, 1.0} and (grid[0] == -1).all() and (grid[:, :, -1] == -1).all()
    inner = vh.contains(hull.lattice_points(axis.numpy().astype(np.float64))).reshape(33, 33, 33)[1:-1, 1:-1, 1:-1]
    assert np.array_equal(grid[1:-1, 1:-1, 1:-1] > 0, inner)


def test_visual_hull_constructors(tmp_path):
    masks, K, poses = hc.sphere_rig(3)
    ref = hull.VisualHull(masks, K, poses)
    assert ref.masks.dtype == np.uint8 and np.array_equal(ref.masks, hull.host_dilate(masks, hull.disk_footprint(12)))
    # the loader's dicts: float masks in [0, 1], with and without a DataLoader's batch dimension; torch tensors or numpy arrays
    loader = [{'img.mask': masks[v].astype(np.float32) / 255.0, 'img.camera_mat': K, 'img.world_mat': poses[v], 'img.scale_mat': np.eye(4)}
              for v in range(3)]
    batched = [dict((k, torch.from_numpy(np.array(a))[None]) for k, a in d.items()) for d in loader]
    for made in (hull.VisualHull.from_loader(loader), hull.VisualHull.from_loader(iter(batched))):
        assert np.array_equal(made.masks, ref.masks) and np.array_equal(made.views, ref.views)
    with pytest.raises(ValueError):
        hull.VisualHull.from_loader([])
    # the dataset's files: params.json with OpenGL poses, mask/view_VV.png
    params, mask_dir = hc.write_dataset(tmp_path, 3)
    made = hull.VisualHull.from_params(params, mask_dir)
    assert np.array_equal(made.masks, ref.masks) and np.array_equal(made.views, ref.views)
    two = hull.VisualHull.from_params(params, mask_dir, views=[3, 1], footprint=hull.diamond_footprint(1))
    assert np.array_equal(two.views, ref.views[[2, 0]]) and two.masks.shape[0] == 2
    with pytest.raises(ValueError):
        hull.VisualHull.from_params(params, mask_dir, views=[4])
    with pytest.raises(ValueError):
        hull.VisualHull(masks, K, poses[:2])
    p = hc.lattice(33)[1][::7]
    assert np.array_equal(ref.contains(p), hull.host_carve_points(p, ref.masks, K, poses)[0])


def _tool(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(root, 'tools', name + '.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_visual_hull_tool_on_the_host(tmp_path, capsys):
    from psnerf_amd.meshcore import load_mesh
    tool = _tool('visual_hull')
    masks, K, poses = hc.sphere_rig(8)
    params, mask_dir = hc.write_dataset(tmp_path, 8)
    out = str(tmp_path / 'hull.ply')
    counts = tool.main(['--cameras', params, '--masks', mask_dir, '--resolution', '32', '--out', out, '--radius', '2', '--host'])
    keep, by = hc.sphere_carve(8, 2)
    assert counts == {'unseen': int((by == -2).sum()), 'kept': int(keep.sum()), 'views': [int((by == v).sum()) for v in range(8)]}
    mesh = load_mesh(out)
    want = hull.VisualHull(masks, K, poses, footprint=hull.disk_footprint(2)).mesh(32, hc.BOX_SIZE)
    assert np.array_equal(mesh.faces, want.faces) and np.array_equal(mesh.vertices, want.vertices.astype(np.float32))
    assert 'view_03' in capsys.readouterr().out


def test_extract_mesh_tool_carves_on_the_host(tmp_path, capsys):
    """tools/extract_mesh.py --carve-masks DIR --cameras params.json: the mesh of Extractor3D(carve=VisualHull.from_params(...))."""
    import os
    import yaml
    from oracle.stage1 import NeuralNetwork
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.meshcore import load_mesh
    from psnerf_amd.stage1.extracting import Extractor3D
    from psnerf_amd.synthetic import stage1_cfg
    tool = _tool('extract_mesh')
    cfg = stage1_cfg('bear')
    cfg['extraction'] = {'resolution': 8, 'upsampling_steps': 2, 'refinement_step': 0}
    exp = tmp_path / 'out' / 'bear' / 'test_1'
    os.makedirs(str(exp / 'models'))
    with open(str(exp / 'config.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f)
    torch.manual_seed(0)
    model = NeuralNetwork(cfg)
    CheckpointIO(str(exp / 'models'), model=model).save('model.pt')
    params, mask_dir = hc.write_dataset(tmp_path, 8)
    args = ['--no-cuda', '--obj_name', 'bear', '--exp_folder', str(tmp_path / 'out'), '--test_out_dir', str(tmp_path / 'test_out'),
            '--mesh_extension', 'ply']
    plain = load_mesh(tool.main(args))
    assert 'carved' not in capsys.readouterr().out
    carved = load_mesh(tool.main(args + ['--carve-masks', mask_dir, '--cameras', params, '--carve-radius', '2']))
    assert 'lattice points carved by the masks of 8 views' in capsys.readouterr().out
    masks, K, poses = hc.sphere_rig(8)
    ex = Extractor3D(model, resolution0=8, upsampling_steps=2, carve=hull.VisualHull(masks, K, poses, footprint=hull.disk_footprint(2)))
    want, stats = ex.generate_mesh()
    assert np.array_equal(carved.faces, want.faces) and np.array_equal(carved.vertices, want.vertices.astype(np.float32).astype(np.float64))
    assert stats['n_points_carved'] > 0 and not np.array_equal(plain.vertices.shape, carved.vertices.shape)
    fewer = load_mesh(tool.main(args + ['--carve-masks', mask_dir, '--cameras', params, '--carve-radius', '2', '--views', '1', '3']))
    assert 'masks of 2 views' in capsys.readouterr().out and len(fewer.faces) > 0
    with pytest.raises(SystemExit):
        tool.main(args + ['--carve-masks', mask_dir])


# ------------------------------------------------------------------------------------------------ C entry points, no GPU needed
def test_hull_entry_points_validate_their_arguments_without_a_gpu():
    from psnerf_amd import hip
    lib = hip._lib
    d = ctypes.c_void_p(64)
    table = (ctypes.c_int32 * 3)(0, 1, 0)

    def refused(rc, word):
        assert rc == hip.E_ARG and word in lib.psn_last_error(), (rc, lib.psn_last_error())

    refused(lib.psn_mask_dilate(None, 1, 4, 4, table, 1, 0, 0, d, d, None), b'null')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, None, 1, 0, 0, d, d, None), b'null')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, table, 1, 0, 0, None, d, None), b'null')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, table, 1, 0, 0, d, None, None), b'null')
    refused(lib.psn_mask_dilate(d, 0, 4, 4, table, 1, 0, 0, d, d, None), b'V=0')
    refused(lib.psn_mask_dilate(d, 1, 0, 4, table, 1, 0, 0, d, d, None), b'H=0')
    refused(lib.psn_mask_dilate(d, 1, 4, 0, table, 1, 0, 0, d, d, None), b'W=0')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, table, -1, 0, 0, d, d, None), b'radius')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, table, hip.HULL_MAX_RADIUS + 1, 0, 0, d, d, None), b'radius')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, table, 1, 2, 0, d, d, None), b'border=2')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, table, 1, -1, 0, d, d, None), b'border=-1')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, table, 1, 0, 2, d, d, None), b'invert')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, (ctypes.c_int32 * 3)(0, -1, 0), 1, 0, 0, d, d, None), b'negative half-width')
    refused(lib.psn_mask_dilate(d, 1, 4, 4, (ctypes.c_int32 * 3)(0, 1, 2), 1, 0, 0, d, d, None), b'above r=1')
    assert lib.psn_mask_dilate_workspace(2, 3, 65) == 2 * 3 * 2 and lib.psn_mask_dilate_workspace(1, 1, 64) == 1
    assert lib.psn_mask_dilate_workspace(0, 3, 3) == -1 and lib.psn_mask_dilate_workspace(1, 0, 3) == -1 and lib.psn_mask_dilate_workspace(1, 3, 0) == -1
    refused(lib.psn_hull_points(None, hip.HULL_F32, 5, d, 1, d, 4, 4, d, d, None), b'null')
    refused(lib.psn_hull_points(d, hip.HULL_F32, 5, None, 1, d, 4, 4, d, d, None), b'null')
    refused(lib.psn_hull_points(d, hip.HULL_F32, 5, d, 1, None, 4, 4, d, d, None), b'null')
    refused(lib.psn_hull_points(d, hip.HULL_F32, 5, d, 1, d, 4, 4, None, d, None), b'null')
    refused(lib.psn_hull_points(d, hip.HULL_F32, 5, d, 1, d, 4, 4, d, None, None), b'null')
    refused(lib.psn_hull_points(d, hip.HULL_F32, 5, d, 0, d, 4, 4, d, d, None), b'V=0')
    refused(lib.psn_hull_points(d, hip.HULL_F32, 5, d, 1, d, 0, 4, d, d, None), b'H=0')
    refused(lib.psn_hull_points(d, hip.HULL_F32, 5, d, 1, d, 4, -3, d, d, None), b'W=-3')
    refused(lib.psn_hull_points(d, 2, 5, d, 1, d, 4, 4, d, d, None), b'point_type')
    refused(lib.psn_hull_points(d, hip.HULL_F64, -1, d, 1, d, 4, 4, d, d, None), b'n_points')
    assert lib.psn_hull_points(None, hip.HULL_F64, 0, d, 1, d, 4, 4, None, None, None) == 0       # nothing to do, nothing launched
    refused(lib.psn_hull_grid(None, 9, d, d, 1, d, 4, 4, -30.0, d, None), b'null')
    refused(lib.psn_hull_grid(d, 9, None, d, 1, d, 4, 4, -30.0, d, None), b'null')
    refused(lib.psn_hull_grid(d, 9, d, None, 1, d, 4, 4, -30.0, d, None), b'null')
    refused(lib.psn_hull_grid(d, 9, d, d, 1, None, 4, 4, -30.0, d, None), b'null')
    refused(lib.psn_hull_grid(d, 9, d, d, 1, d, 4, 4, -30.0, None, None), b'null')
    refused(lib.psn_hull_grid(d, 1, d, d, 1, d, 4, 4, -30.0, d, None), b'n=1')
    refused(lib.psn_hull_grid(d, hip.MESH_MAX_RESOLUTION + 2, d, d, 1, d, 4, 4, -30.0, d, None), b'n=%d' % (hip.MESH_MAX_RESOLUTION + 2))
    refused(lib.psn_hull_grid(d, 9, d, d, 0, d, 4, 4, -30.0, d, None), b'V=0')
    refused(lib.psn_hull_grid(d, 9, d, d, 1, d, 4, 0, -30.0, d, None), b'W=0')
    # the wrappers refuse host tensors like every other product path
    with pytest.raises(RuntimeError):
        hip.mask_dilate(torch.zeros(1, 3, 3, dtype=torch.uint8), [0])
    with pytest.raises(RuntimeError):
        hip.hull_grid(torch.zeros(3, 3, 3), torch.zeros(3, dtype=torch.float64), torch.zeros(1, 16, dtype=torch.float64),
                      torch.zeros(1, 3, 3, dtype=torch.uint8))
