"""Silhouette carving on the GPU (csrc/hull.hip through psnerf_amd/hip.py and psnerf_amd/hull.py) against the numpy definition, byte for
byte: psn_mask_dilate, psn_hull_points, psn_hull_grid, the extractor's ``carve=`` on the device and the hull mesh.  Every output lands
in a buffer with guard zones on both sides (0xFF bytes, NaN floats) that must come back untouched."""
import numpy as np
import pytest
import torch

from tests import hull_cases as hc
from tests.helpers import ATOL_LOGIT, assert_close, stage1_cfg
from psnerf_amd import hull

pytestmark = pytest.mark.gpu
GUARD = 256
SIZES = ((1, 1), (1, 63), (1, 64), (1, 65), (5, 7), (24, 20), (33, 70), (64, 129))


def dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)


def same_bits(t, a):
    """A device tensor and a numpy array of the same dtype hold the same bytes (NaN-safe, -0.0 is not +0.0)."""
    a = np.ascontiguousarray(a)
    h = t.cpu().numpy()
    return h.dtype == a.dtype and h.shape == a.shape and np.array_equal(h.view(np.uint8), a.view(np.uint8))


class Guarded(object):
    """``shape`` elements of ``dtype`` between two guard zones: 0xFF bytes (for floats that is a NaN)."""

    def __init__(self, shape, dtype, cuda):
        n = int(np.prod(shape))
        self.raw = torch.full(((n + 2 * GUARD) * torch.empty(0, dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=cuda)
        self.all = self.raw.view(dtype)
        self.out = self.all[GUARD:GUARD + n].view(shape)

    def intact(self):
        n = self.out.numel()
        edge = torch.cat([self.all[:GUARD], self.all[GUARD + n:]]).contiguous().view(torch.uint8)
        return bool((edge == 0xFF).all())


# ------------------------------------------------------------------------------------------------ psn_mask_dilate
@pytest.mark.parametrize('shape', sorted(hc.SHAPES))
@pytest.mark.parametrize('r', hc.RADII)
def test_mask_dilate_equals_the_definition(cuda, shape, r):
    from psnerf_amd import hip
    fp = hc.SHAPES[shape](r)
    n = 0
    for H, W in SIZES:
        for V in (1, 3):
            for name in hc.PATTERNS:
                m = hc.pattern(name, V, H, W)
                d_m = dev(m, cuda)
                for border in (0, 1):
                    want = hull.host_dilate(m, fp, border)
                    g = Guarded((V, H, W), torch.uint8, cuda)
                    got = hip.mask_dilate(d_m, fp, border, out=g.out)
                    assert same_bits(got, want), '%s(%d), %d x %d x %d, %s, border %d: %d pixels differ' % (
                        shape, r, V, H, W, name, border, int((got.cpu().numpy() != want).sum()))
                    assert g.intact()
                    n += 1
    assert n == len(SIZES) * 2 * len(hc.PATTERNS) * 2


def test_largest_radius_and_a_lopsided_footprint(cuda):
    """r = PSN_HULL_MAX_RADIUS (half-widths of 64: the three-word window is used to its last bit) and a table that is not symmetric in
    dy, with half-widths that differ from row to row."""
    from psnerf_amd import hip
    g = np.random.RandomState(3)
    lopsided = np.array([0, 5, 1, 5, 0, 2, 3, 4, 5, 0, 1], dtype=np.int32)
    for fp in (hull.disk_footprint(hip.HULL_MAX_RADIUS), hull.diamond_footprint(hip.HULL_MAX_RADIUS), np.full(2 * 64 + 1, 64, dtype=np.int32), lopsided):
        for H, W in ((3, 200), (70, 129), (140, 64)):
            m = (g.rand(2, H, W) < 0.003).astype(np.uint8)
            for border in (0, 1):
                assert same_bits(hull.dilate_masks(dev(m, cuda), fp, border), hull.host_dilate(m, fp, border)), (len(fp), H, W, border)
            assert same_bits(hull.erode_masks(dev(1 - m, cuda), fp), hull.host_erode(1 - m, fp))


def test_erosion_and_mask_valid_equal_their_definitions(cuda):
    for H, W in SIZES:
        for name in hc.PATTERNS:
            m = hc.pattern(name, 3, H, W)
            d_m = dev(m, cuda)
            for shape in sorted(hc.SHAPES):
                for r in hc.RADII:
                    fp = hc.SHAPES[shape](r)
                    assert same_bits(hull.erode_masks(d_m, fp), hull.host_erode(m, fp)), (shape, r, H, W, name)
            for it in (1, 2):
                valid = hull.mask_valid(d_m, it)
                assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), hull.mask_valid(m, it))
            assert np.array_equal(hull.mask_valid(d_m[0] != 0).cpu().numpy(), hull.mask_valid(m[0]))     # one bool mask [H, W]


# ------------------------------------------------------------------------------------------------ psn_hull_points
def _scene(V, H=24, W=20, seed=0):
    """V random cameras around the origin with blotchy masks (random pixels dilated by disk(2): about half of each image is set)."""
    cams = [hc.random_camera(100 * seed + v, H, W) for v in range(V)]
    K = np.stack([c[0] for c in cams])
    poses = np.stack([c[1] for c in cams])
    seeds = np.random.RandomState(seed).rand(V, H, W) < 0.06
    return hull.host_dilate(seeds, hull.disk_footprint(2)) * np.uint8(255), K, poses


def _check_points(cuda, p, masks, K, poses):
    from psnerf_amd import hip
    want_keep, want_by = hull.host_carve_points(p, masks, K, poses)
    Q = p.shape[0]
    gk, gb = Guarded((Q,), torch.uint8, cuda), Guarded((Q,), torch.int32, cuda)
    views = torch.from_numpy(hull._views(K, poses, masks.shape[0])).to(cuda)
    keep, by = hip.hull_points(dev(p, cuda), views, dev(masks, cuda), out=(gk.out, gb.out))
    assert same_bits(by, want_by), '%d of %d points differ' % (int((by.cpu().numpy() != want_by).sum()), Q)
    assert same_bits(keep, want_keep.astype(np.uint8)) and gk.intact() and gb.intact()
    return want_by


@pytest.mark.parametrize('V', [1, 2, 5, 31, 32, 33, 65])
def test_hull_points_equal_the_definition(cuda, V):
    """V around PSN_HULL_VIEW_CHUNK = 32 (one chunk less one, one chunk, one chunk and one view) and two chunks and one."""
    from psnerf_amd import hip
    assert hip.HULL_VIEW_CHUNK == 32
    masks, K, poses = _scene(V, seed=V)
    g = np.random.RandomState(V)
    seen = set()
    for Q in (1, 63, 64, 65, 1000):
        p = (g.rand(Q, 3) - 0.5) * 1.2
        p[::7] *= 4.0                                                   # (some far outside every image)
        for dtype in (np.float32, np.float64):
            seen.update(_check_points(cuda, p.astype(dtype), masks, K, poses).tolist())
    assert -1 in seen and max(seen) >= 0
    if V >= 33:
        assert max(seen) >= 32                                          # (a view of a later chunk carved first)


def test_hull_points_constructed(cuda):
    """Behind the camera, at its centre, NaN; and, with an axis-aligned camera with power-of-two intrinsics (every product exact),
    points whose u + 0.5 (v + 0.5) is exactly 0, just below 0, exactly W (H) and just below."""
    H, W = 16, 32
    K, c2w = hc.axis_camera(H, W)
    edge, inside = hc.edge_points(H, W)
    p = np.concatenate([hc.odd_points(c2w), edge])
    for fill, expect in ((255, -1), (0, 0)):
        masks = np.full((1, H, W), fill, dtype=np.uint8)
        by = _check_points(cuda, p, masks, K, c2w[None])
        assert by[:5].tolist() == [-2, -2, -2, -2, expect] and np.array_equal(by[5:] == expect, inside) and (by[5:][~inside] == -2).all()
    masks = np.full((1, H, W), 255, dtype=np.uint8)                    # only the four border pixels the edge points fall on are background
    masks[0, 3, 0] = masks[0, 3, W - 1] = masks[0, 0, 5] = masks[0, H - 1, 5] = 0
    by = _check_points(cuda, p, masks, K, c2w[None])
    assert by[5:].tolist() == [0, -2, -2, 0, 0, -2, -2, 0]
    masks2, K2, poses2 = _scene(3, seed=9)
    for v in range(3):
        _check_points(cuda, hc.odd_points(poses2[v]), masks2, K2, poses2)
        _check_points(cuda, hc.odd_points(poses2[v]).astype(np.float32), masks2, K2, poses2)


@pytest.mark.parametrize('V', [1, 3, 8])
def test_hull_points_on_the_sphere_rigs(cuda, V):
    masks, K, poses = hc.sphere_rig(V)
    axis, p = hc.lattice(33)
    for radius in (1, 2, 12):
        vh = hull.VisualHull(dev(masks, cuda), K, poses, footprint=hull.disk_footprint(radius))
        assert same_bits(vh.masks, hull.host_dilate(masks, hull.disk_footprint(radius)))
        keep, by = vh.carve_points(dev(p, cuda))
        want_keep, want_by = hc.sphere_carve(V, radius)
        assert same_bits(by, want_by) and keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want_keep)
        assert np.array_equal(vh.contains(dev(p.astype(np.float32), cuda)).cpu().numpy(),
                              hull.host_carve_points(p.astype(np.float32), vh.masks.cpu().numpy(), K, poses)[0])
    # host masks (any non-zero value is set) beside device points: moved, not refused
    by = hull.carve_points(dev(p, cuda), hull.host_dilate(masks, hull.disk_footprint(2)) * np.uint8(7), K, poses)[1]
    assert same_bits(by, hc.sphere_carve(V, 2)[1])


# ------------------------------------------------------------------------------------------------ psn_hull_grid
@pytest.mark.parametrize('n', [2, 9, 33, 65])
@pytest.mark.parametrize('V', [1, 5])
def test_hull_grid_equals_the_definition(cuda, n, V):
    from psnerf_amd import hip
    masks, K, poses = hc.sphere_rig(V)
    dil = hull.host_dilate(masks, hull.disk_footprint(2))
    axis = hc.BOX_SIZE * torch.linspace(-0.5, 0.5, n)
    keep = hull.host_carve_points(hull.lattice_points(axis.numpy().astype(np.float64)), dil, K, poses)[0].reshape(n, n, n)
    views = torch.from_numpy(hull._views(K, poses, V)).to(cuda)
    d_axis, d_masks = axis.to(torch.float64).to(cuda), dev(dil, cuda)
    for field in ('random', 'sphere'):
        grid = np.random.RandomState(n + V).randn(n, n, n).astype(np.float32) if field == 'random' else hc.sphere_field(n)
        kept = np.argwhere(keep)
        if len(kept) >= 2:                                              # among the untouched elements: -0.0 and a NaN with a payload
            grid[tuple(kept[0])] = np.float32(-0.0)
            grid.view(np.uint32)[tuple(kept[-1])] = 0x7FC01234
        want = grid.copy()
        want_count = hull.host_carve_grid(want, axis, dil, K, poses)
        assert want_count == int((~keep).sum()) and (n == 2 or 0 < want_count < n ** 3)
        runs = []
        for _ in range(2):
            g = Guarded((n, n, n), torch.float32, cuda)
            g.out.copy_(dev(grid, cuda))
            count = hip.hull_grid(g.out, d_axis, views, d_masks)
            assert count.dtype == torch.int64 and int(count.item()) == want_count
            assert same_bits(g.out, want), '%d^3, %d views, %s: %d elements differ' % (
                n, V, field, int((g.out.cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum()))
            assert g.intact()
            runs.append(g.out.clone())
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
        # the public entry: another value, the same set
        d_grid = dev(grid, cuda)
        assert hull.carve_grid(d_grid, axis, d_masks, K, poses, value=7.5) == want_count
        assert bool((d_grid.cpu().numpy()[~keep] == 7.5).all()) and same_bits(d_grid[dev(keep, cuda)], grid[keep])


# ------------------------------------------------------------------------------------------------ the extractor and the hull mesh
def _networks(seed=0):
    import psnerf_amd.stage1 as s1
    from oracle import stage1 as o1
    cfg = stage1_cfg('bear')
    torch.manual_seed(seed)
    onet = o1.NeuralNetwork(cfg)
    net = s1.NeuralNetwork(cfg)
    net.load_state_dict(onet.state_dict())
    return net, onet


def test_extractor_carves_on_the_device(cuda):
    """resolution0 = 16, one upsampling step, the sphere-initialised network: the device's carved grid against the host path's (the CPU
    oracle through the numpy definitions) under the gate of test_mesh_gpu's device-versus-host test on the values (1e-4 relative,
    ATOL_LOGIT absolute, at the points both paths evaluated), and exactly on the carved set and its count."""
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D
    net, onet = _networks()
    net = net.to(cuda)
    masks, K, poses = hc.sphere_rig(8)
    fp = hull.disk_footprint(2)
    kw = dict(resolution0=16, upsampling_steps=1)
    host = Extractor3D(onet, carve=hull.VisualHull(masks, K, poses, footprint=fp), **kw)
    hmesh, hstats = host.generate_mesh()
    ops.reset_hits()
    with ops.strict():
        ex = Extractor3D(net, device=cuda, carve=hull.VisualHull(dev(masks, cuda), K, poses, footprint=fp), **kw)
        ex.phase_events = []
        mesh, stats = ex.generate_mesh()
        plain = Extractor3D(net, device=cuda, **kw)
        mesh0, stats0 = plain.generate_mesh()
        none = Extractor3D(net, device=cuda, carve=None, **kw)
        mesh1, stats1 = none.generate_mesh()
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    grid, hgrid = ex.last_grid.cpu().numpy(), host.last_grid
    carved, hcarved = grid == np.float32(-30.0), hgrid == np.float32(-30.0)
    n = 33
    keep = hc.sphere_carve(8, 2)[0].reshape(n, n, n)
    assert np.array_equal(carved, ~keep) and np.array_equal(hcarved, ~keep)
    assert stats['n_points_carved'] == hstats['n_points_carved'] == int((~keep).sum()) and stats['time (carve)'] >= 0.0
    assert [name for name, _, _ in ex.phase_events].count('carve') == 1
    both = keep & ex.last_known.cpu().numpy() & host.last_known
    assert int(both.sum()) > 1000
    assert_close(torch.from_numpy(grid[both]), torch.from_numpy(hgrid[both]), 1e-4, 'carved extraction: -logit of the evaluated points', atol=ATOL_LOGIT)
    assert same_bits(ex.last_grid[dev(keep, cuda)], plain.last_grid.cpu().numpy()[keep])        # what is not carved keeps its bits
    assert len(mesh.faces) > 100 and len(hmesh.faces) > 100
    # carve=None: every stat and result is what it was
    assert np.array_equal(mesh1.vertices, mesh0.vertices) and np.array_equal(mesh1.faces, mesh0.faces)
    assert same_bits(none.last_grid, plain.last_grid.cpu().numpy()) and sorted(stats1) == sorted(stats0) and 'n_points_carved' not in stats0
    # the masks of a host-side hull are moved to the grid's device once
    moved = Extractor3D(net, device=cuda, carve=hull.VisualHull(masks, K, poses, footprint=fp), **kw)
    moved.generate_mesh()
    assert same_bits(moved.last_grid, grid) and moved.carve.masks.is_cuda


def test_hull_mesh_on_the_device_equals_the_host_path(cuda):
    from psnerf_amd import meshclean
    masks, K, poses = hc.sphere_rig(8)
    host = hull.VisualHull(masks, K, poses).mesh(32, hc.BOX_SIZE)
    vh = hull.VisualHull(dev(masks, cuda), K, poses)
    mesh = vh.mesh(32, hc.BOX_SIZE)
    assert np.array_equal(mesh.faces, host.faces) and np.abs(mesh.vertices - host.vertices).max() <= 1e-12 * hc.BOX_SIZE / 32
    assert np.linalg.norm(mesh.vertices, axis=1).min() >= hc.SPHERE_RADIUS - hc.BOX_SIZE / 32
    assert len(meshclean.components(dev(mesh.vertices, cuda), dev(mesh.faces, cuda))[1]['label']) == 1
    grid, _ = vh.indicator(32, hc.BOX_SIZE)
    assert same_bits(grid, hull.VisualHull(masks, K, poses).indicator(32, hc.BOX_SIZE)[0])
    # the loader's dicts (float masks in [0, 1]) straight onto the device
    loader = [{'img.mask': masks[v] / np.float32(255.0), 'img.camera_mat': K, 'img.world_mat': poses[v]} for v in range(8)]
    made = hull.VisualHull.from_loader(loader, device=cuda)
    assert made.masks.is_cuda and same_bits(made.masks, vh.masks.cpu().numpy()) and np.array_equal(made.views, vh.views)


# ------------------------------------------------------------------------------------------------ argument errors
def test_bad_arguments_are_refused_before_any_launch(cuda):
    from psnerf_amd import hip
    from tests.test_hull_cpu import test_hull_entry_points_validate_their_arguments_without_a_gpu as entry_points
    entry_points()
    m = torch.zeros(1, 4, 4, dtype=torch.uint8, device=cuda)
    for table, border, word in (([0, 1, 0], 2, 'border=2'), ([0, -1, 0], 0, 'negative half-width'), ([0, 2, 0], 0, 'above r=1'),
                                ([0] * (2 * hip.HULL_MAX_RADIUS + 3), 0, 'radius')):
        with pytest.raises(RuntimeError, match=word):
            hip.mask_dilate(m, table, border)
    with pytest.raises(RuntimeError, match='2 r \\+ 1'):
        hip.mask_dilate(m, [0, 1], 0)
    views = torch.zeros(1, 16, dtype=torch.float64, device=cuda)
    one = torch.zeros(1, 1, 1, device=cuda)
    with pytest.raises(RuntimeError, match='n=1'):
        hip.hull_grid(one, torch.zeros(1, dtype=torch.float64, device=cuda), views, m)
    assert float(one.sum()) == 0.0
    for bad in (lambda: hip.hull_grid(torch.zeros(3, 3, 2, device=cuda), torch.zeros(3, dtype=torch.float64, device=cuda), views, m),
                lambda: hip.hull_grid(torch.zeros(3, 3, 3, device=cuda), torch.zeros(3, device=cuda), views, m),
                lambda: hip.hull_grid(torch.zeros(3, 3, 3, device=cuda), torch.zeros(3, dtype=torch.float64, device=cuda), views[:, :15], m),
                lambda: hip.hull_points(torch.zeros(4, 3, dtype=torch.float16, device=cuda), views, m),
                lambda: hip.hull_points(torch.zeros(4, 2, device=cuda), views, m),
                lambda: hip.hull_points(torch.zeros(4, 3, device=cuda), views, m[:0]),
                lambda: hip.mask_dilate(m.to(torch.float32), [0], 0)):
        with pytest.raises(RuntimeError):
            bad()
    keep, by = hip.hull_points(torch.zeros(0, 3, device=cuda), views, m)     # no points: no launch, empty outputs
    assert keep.shape == (0,) and by.shape == (0,)
