"""The view projection on the GPU (csrc/meshproject.hip through psnerf_amd/meshproject.py, meshdist.MeshIndex.project_rows,
meshbake.bake_views and mesheval.evaluate_mesh) against the float64 numpy definition meshproject.host_project_rows, on the cases of
tests/project_cases.py.

What is demanded, and why.  EVERY output must be equal: the kernel runs the definition's projection, footprint, facing and mask tests
and forms the segment to each camera by a fixed sequence of correctly rounded float64 + - x / sqrt in the definition's order with
contraction off; it walks the segment with the function psn_ray_cast instantiates, which loses no triangle
(tests/test_raycast_gpu.py holds it to that); a row's views accumulate in one thread in ascending order.  So n_seen, best_view and
words are compared exactly and sum, sum_sq, weight and best_value bit for bit.  A mismatch is a finding about the order of operations
or the walk, not a tolerance to widen.  Outputs land in guarded buffers (NaN / a sentinel), so a row the kernel skips shows."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from tests import bake_cases as bc, hull_cases as hc, occlusion_cases as oc, project_cases as pc
from tests.test_mesheval_gpu import EXACT, GATE, MEANS
from psnerf_amd import meshbake as mb
from psnerf_amd import meshdist as md
from psnerf_amd import meshproject as mp
from psnerf_amd.meshcore import Mesh

pytestmark = pytest.mark.gpu
SENTINEL = -77
FIELDS = mp.Projection._fields


def dev(x, cuda):
    return None if x is None else torch.from_numpy(np.array(x)).to(cuda)                 # (a copy: the cases are read-only)


def same_bits(got, want):
    if got is None or want is None:
        return got is None and want is None
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return np.array_equal(got.view(np.uint64), want.view(np.uint64)) if got.dtype == np.float64 else np.array_equal(got, want)


def guards(R, V, C, cuda, bits=True):
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float64, device=cuda)
    mark = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=cuda)
    return (nan(R, C) if C else None, nan(R, C) if C else None, nan(R), mark(R), mark(R), nan(R, C) if C else None,
            mark(R, (V + 31) // 32) if bits else None)


def index_of(c, name, cuda):
    """The MeshIndex of a case; for the all-oversize case the grid of small cells with max_span = 1 (tests/test_occlusion_gpu.py)."""
    if 'every face oversize' not in name:
        return md.MeshIndex(c['v'], c['f'], device=cuda)
    index = md.MeshIndex(c['v'], c['f'], device=cuda, cell=oc.ALL_OVERSIZE_CELL, max_span=1)
    assert index.n_entries == 0 and int(index.cell_start.sum()) == 0 and index.n_over == len(index.over_list) == len(c['f'])
    return index


def differing(got, want):
    return ', '.join('%s: %d rows' % (k, int((np.asarray(g.cpu().numpy() != w).reshape(len(w), -1)).any(axis=1).sum()))
                     for k, g, w in zip(FIELDS, got, want) if g is not None and not same_bits(g, w))


@pytest.mark.parametrize('name', list(pc.CASES))
def test_device_against_the_definition(cuda, name):
    c = pc.case(name)
    R, V, C = len(c['points']), c['V'], c['C']
    index = index_of(c, name, cuda)
    if 'two oversize' in name:
        assert index.n_over == 2
    p, n, views, img, masks = (dev(c[k], cuda) for k in ('points', 'normals', 'views', 'images', 'masks'))
    want = c['want']
    kw = dict(hw=c['hw'], masks=masks, bias=c['bias'], cos_min=c['cos_min'], weight=c['weight'], frame=c['frame'])
    n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
    out = guards(R, V, C, cuda)
    got = index.project_rows(p, n, img, views, bits=True, n_tests=n_tests, out=out, **kw)
    assert all((g is None and o is None) or g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    seen = int(want.n_seen.sum())
    print('%s: F=%d, %d rows x %d views, %d seen pairs, %d rows unseen, %.1f tests per (row, view)' % (
        name, len(c['f']), R, V, seen, int((want.n_seen == 0).sum()), n_tests.item() / (R * V)))
    assert all(same_bits(g, w) for g, w in zip(got, want)), differing(got, want)
    assert (want.n_seen[c['dead']] == 0).all() and (R < 63 or c['dead'].sum() == 5) and seen > 0
    # without the bits: the same six, no words; and through the public function on device tensors and on a numpy mesh with device=
    plain = index.project_rows(p, n, img, views, out=guards(R, V, C, cuda, bits=False), **kw)
    assert plain.words is None and all(same_bits(a, b) for a, b in zip(plain[:6], want[:6]))
    public = mp.project_rows(index, p, n, img, c['K'], c['poses'], masks=masks, bias=c['bias'], cos_min=c['cos_min'], weight=c['weight'],
                             frame=c['frame'], bits=True, hw=c['hw'])
    assert all(x is None or x.is_cuda for x in public) and all(same_bits(a, b) for a, b in zip(public, want))
    # two runs, the second on an index built again (its lists may come out in another order), give the same bits
    again = index_of(c, name, cuda).project_rows(p.clone(), n.clone(), img, views, bits=True, **kw)
    assert all(same_bits(a, None if b is None else b.cpu().numpy()) for a, b in zip(again, got))


def test_default_bias_and_host_inputs(cuda):
    """project_rows(device='cuda') on numpy inputs: the default bias is the host's, images and masks are uploaded, the result equals."""
    name = 'icosphere, R 257, V 33, u8 C3, masks'
    c = pc.case(name)
    got = mp.project_rows((c['v'], c['f']), c['points'], c['normals'], c['images'], c['K'], c['poses'], masks=c['masks'], bits=True, device=cuda)
    assert all(x.is_cuda for x in got) and all(same_bits(a, b) for a, b in zip(got, c['want']))
    helpers = [(f(got).cpu().numpy(), f(c['want'])) for f in (mp.mean, mp.spread)]
    assert all(np.allclose(a, b, rtol=0, atol=1e-15) for a, b in helpers)


def test_against_materialised_rays(cuda):
    """The same candidate segments written out and handed to MeshIndex.ray_cast(any_hit=True): the same blocked pairs, and the fused
    kernel makes no more ray-triangle tests than psn_ray_cast does on them (it is the same walk)."""
    from psnerf_amd import hip, hull
    c = pc.case('marching cubes, R 63, V 33, f32 C3, camera normals, uniform')
    p, n = c['points'][~c['dead']], c['normals'][~c['dead']]
    index = md.MeshIndex(c['v'], c['f'], device=cuda)
    H, W = c['hw']
    origins, directions, pairs = [], [], []
    for view in range(c['V']):
        pu, pv, front = hull._project_uv(p, c['views'][view])
        o = c['views'][view, 9:12]
        e = o[None] - p
        cosine = ((n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]) / np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        with np.errstate(invalid='ignore'):
            cand = np.nonzero(front & (pu >= 0) & (pu <= W - 1) & (pv >= 0) & (pv <= H - 1) & (cosine > 0))[0]
        x0, y0 = np.floor(pu[cand]).astype(int), np.floor(pv[cand]).astype(int)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        m = c['masks'][view] != 0
        cand = cand[m[y0, x0] & m[y0, x1] & m[y1, x0] & m[y1, x1]]
        q = p[cand] + c['bias'] * n[cand]
        origins.append(q)
        directions.append(o[None] - q)
        pairs.append(np.stack([cand, np.full(len(cand), view)], axis=1))
    od, dd, pairs = dev(np.concatenate(origins), cuda), dev(np.concatenate(directions), cuda), np.concatenate(pairs)
    hit = index.ray_cast(od, dd, 0.0, 1.0, any_hit=True)[3].cpu().numpy()
    seen = np.zeros((len(p), c['V']), dtype=bool)
    seen[pairs[~hit, 0], pairs[~hit, 1]] = True
    n_fused, n_rays = torch.zeros(1, dtype=torch.int64, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda)
    got = index.project_rows(dev(p, cuda), dev(n, cuda), None, dev(c['views'], cuda), hw=c['hw'], masks=dev(c['masks'], cuda), bias=c['bias'],
                             bits=True, n_tests=n_fused)
    hip.ray_cast(index.index, od, dd, 0.0, 1.0, any_hit=True, n_tests=n_rays)
    print('%d candidate segments, %d blocked; tests: fused %d, materialised %d' % (len(pairs), int(hit.sum()), n_fused.item(), n_rays.item()))
    assert np.array_equal(mp.unpack_bits(got.words, c['V']), seen) and 0 < hit.sum() < len(hit)
    assert 0 < int(n_fused.item()) <= int(n_rays.item())


def test_vertex_views_and_face_visibility_on_the_device(cuda):
    v, f = pc.sphere(2)
    H, W = pc.H, pc.W
    K, poses = pc.cameras(v, 7, H, W, seed=3)
    img, masks = pc.images(7, H, W, 3, np.float32, seed=3), pc.masks_for(7, H, W, seed=3)
    host = mp.vertex_views((v, f), img, K, poses, masks=masks, bits=True, frame='camera_normal')
    got = mp.vertex_views((v, f), img, K, poses, masks=masks, bits=True, frame='camera_normal', device=cuda)
    assert all(x.is_cuda for x in got) and got.n_seen.shape == (len(v),) and 0 < int(host.n_seen.sum())
    assert all(same_bits(a, b) for a, b in zip(got, host))
    on_device = mp.vertex_views((dev(v, cuda), dev(f, cuda)), dev(img, cuda), K, poses, masks=dev(masks, cuda), bits=True, frame='camera_normal')
    assert all(same_bits(a, b) for a, b in zip(on_device, host))
    assert np.array_equal(mp.fused_normals(got).cpu().numpy() != 0, mp.fused_normals(host) != 0)
    # faces: the device's rows are the host's bit for bit, and so are the counts; trimming gives the same mesh
    K, poses = pc.cameras(v, 3, H, W, seed=4)
    rows_d, rows_h = mp.face_rows(dev(v, cuda), dev(f, cuda)), mp.face_rows(v, f)
    assert same_bits(rows_d[0], rows_h[0]) and same_bits(rows_d[1], rows_h[1])
    n_seen = mp.face_visibility((v, f), K, poses, H, W)
    assert same_bits(mp.face_visibility((v, f), K, poses, H, W, device=cuda), n_seen) and 0 < (n_seen > 0).sum() < len(f)
    t_host, _ = mp.trim_unseen(Mesh(v, f), K, poses, H, W)
    t_dev, seen = mp.trim_unseen(Mesh(v, f), K, poses, H, W, device=cuda)
    assert same_bits(seen, n_seen) and np.array_equal(t_dev.vertices, t_host.vertices) and np.array_equal(t_dev.faces, t_host.faces)


@pytest.mark.parametrize('name', ['icosphere(1)', 'a tetrahedron', 'zero-area faces'])
def test_bake_views_on_the_device(cuda, name):
    """bake_views at T = 64 on a mesh of tests/bake_cases.py: the device bake, in one chunk and in several, equals the host bake bit for
    bit -- every texel of all four maps, the fill included."""
    from psnerf_amd import ops
    v, f, vn = bc.meshes()[name]
    mesh = (v, f) if vn is None else (v, f, vn)
    H, W = 40, 32
    K, poses = pc.cameras(v, 5, H, W, seed=1)
    img, masks = pc.images(5, H, W, 3, np.uint8, seed=4), pc.masks_for(5, H, W, seed=4)
    host = mb.bake_views(mesh, img, K, poses, size=64, masks=masks, fill=0.25)
    ops.reset_hits()
    with ops.strict():
        d_mesh = tuple(dev(x, cuda) for x in mesh)
        one = mb.bake_views(d_mesh, dev(img, cuda), K, poses, size=64, masks=dev(masks, cuda), fill=0.25)
        parts = mb.bake_views(mesh, img, K, poses, atlas=host['atlas'], masks=masks, fill=0.25, chunk_faces=max(1, len(f) // 3), device=cuda)
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    for baked in (one, parts):
        assert baked['photo'].is_cuda and baked['photo'].dtype == torch.float32 and baked['seen'].shape == (64, 64, 1)
        for key in ('photo', 'photo_best', 'seen', 'spread'):
            got, want = baked[key].cpu().numpy(), host[key]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), '%s: %d texels differ' % (key, int((got != want).sum()))
    owned = host['atlas'].owner()[0] >= 0
    print('%s: views per owned texel %.0f .. %.0f' % (name, host['seen'][owned].min(), host['seen'][owned].max()))


def test_evaluate_mesh_visible_from_on_the_device(cuda):
    """evaluate_mesh(visible_from=) on the device against the host path from an equal rng state: the kept samples and every integer
    equal, the means within the gate of tests/test_mesheval_gpu.py."""
    from psnerf_amd.mesheval import evaluate_mesh
    pred, gt = Mesh(*pc.sphere(2)), Mesh(*pc.sphere(3))
    _, K, poses = hc.sphere_rig(12)
    visible_from = (K, poses[:5], hc.RIG_H, hc.RIG_W)
    host = evaluate_mesh(pred, gt, 1500, iou_points=2000, rng=np.random.RandomState(7), visible_from=visible_from)
    got = evaluate_mesh(pred, gt, 1500, iou_points=2000, rng=np.random.RandomState(7), visible_from=visible_from, device=cuda)
    assert set(got) == set(host) and 0.0 < host['visible_fraction_pred'] < 1.0 and 0.0 < host['visible_fraction_gt'] < 1.0
    for side in ('pred', 'gt'):
        assert got['raw'][side + '_visible'].is_cuda and np.array_equal(got['raw'][side + '_visible'].cpu().numpy(), host['raw'][side + '_visible'])
        assert got['visible_fraction_' + side] == host['visible_fraction_' + side]
    for key in EXACT:
        assert got[key] == host[key], key
    for key in MEANS:
        print('    %s: %.17g / %.17g' % (key, got[key], host[key]))
        assert abs(got[key] - host[key]) <= GATE * abs(host[key]), key


def test_c_abi_errors(cuda):
    """Every argument check returns its error without launching: bad arguments only."""
    from psnerf_amd import hip
    c = pc.case('icosphere, one row, one view, f32 C1')
    index = md.MeshIndex(c['v'], c['f'], device=cuda)
    H, W = 8, 8
    p = torch.zeros(10, 3, dtype=torch.float64, device=cuda)
    n = torch.ones(10, 3, dtype=torch.float64, device=cuda)
    views = lambda V: dev(np.tile(c['views'][:1], (V, 1)) if V else np.zeros((0, 16)), cuda)
    image = lambda V, C=3, dtype=torch.float32: torch.zeros(V, H, W, C, dtype=dtype, device=cuda)
    call = lambda p, n, v, img, **kw: hip.project_rows(index.index, p, n, v, img, **kw)
    assert bool((call(p, n, views(256), image(256))[3] == 0).all())                  # rows at the centre of the sphere: no view sees them
    wide = torch.ones(10, 6, dtype=torch.float64, device=cuda)
    for bad in (lambda: call(p, n, views(0), image(1)), lambda: call(p, n, views(257), image(257)), lambda: call(p.cpu(), n, views(2), image(2)),
                lambda: call(p, n.float(), views(2), image(2)), lambda: call(p[:5], n, views(2), image(2)),
                lambda: call(wide[:, ::2], n, views(2), image(2)), lambda: call(p, n, views(2), image(3)),
                lambda: call(p, n, views(2), image(2, 5)), lambda: call(p, n, views(2), image(2, dtype=torch.float64)),
                lambda: call(p, n, views(2), image(2).cpu()), lambda: call(p, n, views(2), None),
                lambda: call(p, n, views(2), image(2), hw=(H, W + 1)), lambda: call(p, n, views(2), image(2), bias=float('inf')),
                lambda: call(p, n, views(2), image(2), cos_min=float('nan')), lambda: call(p, n, views(2), image(2, 4), camera_normal=True),
                lambda: call(p, n, views(2), None, hw=(H, W), camera_normal=True),
                lambda: call(p, n, views(2), None, hw=(0, W)), lambda: call(p, n, views(2), None, hw=(H, 32769)),
                lambda: call(p, n, views(2), image(2), masks=torch.ones(2, H, W + 1, dtype=torch.uint8, device=cuda)),
                lambda: call(p, n, views(2), image(2), masks=torch.ones(2, H, W, dtype=torch.int32, device=cuda)),
                lambda: call(p, n, torch.zeros(2, 12, dtype=torch.float64, device=cuda), image(2)),
                lambda: call(p, n, views(2), image(2), out=guards(9, 2, 3, cuda, bits=False)),
                lambda: call(p, n, views(2), None, hw=(H, W), out=guards(10, 2, 3, cuda, bits=False))):
        with pytest.raises(RuntimeError, match='project_rows'):
            bad()
    empty = call(p[:0], n[:0], views(33), image(33, 4), bits=True)
    assert empty[0].shape == (0, 4) and empty[2].shape == (0,) and empty[5].shape == (0, 4) and empty[6].shape == (0, 2) and empty[3].is_cuda
    bare = call(p, n, views(2), None, hw=(H, W))
    assert bare[0] is None and bare[1] is None and bare[5] is None and bare[3].shape == (10,)
    # null pointers and bad modes, which the wrapper cannot produce: the entry point itself
    out = guards(10, 2, 3, cuda)
    v2, img2 = views(2), image(2)
    mask2 = torch.ones(2, H, W, dtype=torch.uint8, device=cuda)
    args = collections.OrderedDict([('index', ctypes.byref(index.index)), ('points', p.data_ptr()), ('normals', n.data_ptr()), ('n_rows', 10),
                                    ('views', v2.data_ptr()), ('n_views', 2), ('images', img2.data_ptr()), ('image_type', hip.IMG_F32), ('H', H),
                                    ('W', W), ('C', 3), ('masks', mask2.data_ptr()), ('bias', 0.0), ('cos_min', 0.0),
                                    ('weight_mode', hip.PROJECT_WEIGHT_COSINE), ('frame_mode', hip.PROJECT_FRAME_RAW), ('sum', out[0].data_ptr()),
                                    ('sum_sq', out[1].data_ptr()), ('weight', out[2].data_ptr()), ('n_seen', out[3].data_ptr()),
                                    ('best_view', out[4].data_ptr()), ('best_value', out[5].data_ptr()), ('words', out[6].data_ptr()),
                                    ('n_tests', None), ('stream', None)])
    assert hip._lib.psn_project_rows(*args.values()) == 0
    torch.cuda.synchronize()
    assert bool((out[3] == 0).all()) and bool((out[4] == -1).all()) and bool((out[0] == 0).all()) and bool((out[6] == 0).all())
    for key, value in (('index', None), ('vertices', None), ('faces', None), ('cell_start', None), ('points', None), ('normals', None),
                       ('views', None), ('images', None), ('sum', None), ('sum_sq', None), ('weight', None), ('n_seen', None), ('best_view', None),
                       ('best_value', None), ('n_views', 0), ('n_views', 257), ('n_rows', -1), ('C', 0), ('C', 5), ('C', -1), ('H', 0), ('H', 32769),
                       ('W', 0), ('W', 32769), ('image_type', 2), ('image_type', -1), ('weight_mode', 2), ('weight_mode', -1), ('frame_mode', 2),
                       ('frame_mode', -1), ('bias', float('nan')), ('bias', float('inf')), ('cos_min', float('nan')), ('cos_min', -float('inf'))):
        broken = collections.OrderedDict(args)
        if key in broken:
            broken[key] = value
        else:                                                            # a field of the index: one changed in a copy of the struct
            ix = hip.PsnMeshIndex.from_buffer_copy(index.index)
            setattr(ix, key, value)
            broken['index'] = ctypes.byref(ix)
        assert hip._lib.psn_project_rows(*broken.values()) == hip.E_ARG, '%s = %r' % (key, value)
        assert b'project_rows' in hip._lib.psn_last_error()
    for C in (1, 4):                                                     # camera normals need three channels
        broken = collections.OrderedDict(args, frame_mode=hip.PROJECT_FRAME_CAMERA_NORMAL, C=C)
        assert hip._lib.psn_project_rows(*broken.values()) == hip.E_ARG and b'camera_normal' in hip._lib.psn_last_error()
    assert hip._lib.psn_project_rows(*collections.OrderedDict(args, n_rows=0, points=None, normals=None, sum=None).values()) == 0
    assert hip._lib.psn_project_rows(*collections.OrderedDict(args, images=None, C=0, sum=None, sum_sq=None, best_value=None, masks=None,
                                                              words=None).values()) == 0
    torch.cuda.synchronize()
