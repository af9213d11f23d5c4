"""Occlusion on the GPU (csrc/meshocclude.hip through psnerf_amd/meshocclude.py, meshdist.MeshIndex.occlusion and meshbake.bake_occlusion)
against the float64 numpy definition meshocclude.host_occlusion_rows, on the cases of tests/occlusion_cases.py.

What is demanded, and why.  EVERY output must be equal: the kernel forms each ray from (point, normal, table) by a fixed sequence of
correctly rounded float64 + - x / in the definition's order with contraction off, so its rays are the definition's bit for bit; it
walks them with the function psn_ray_cast instantiates, which loses no triangle (tests/test_raycast_gpu.py holds it to that); counts
are integers and the bent normal is a sum in index order.  So hits, visible and words are compared exactly and ao and bent bit for
bit.  A mismatch is a finding about the order of operations or the walk, not a tolerance to widen.  Outputs land in guarded buffers
(NaN / a sentinel), so a row the kernel skips shows."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from tests import bake_cases as bc, occlusion_cases as oc
from psnerf_amd import meshbake as mb
from psnerf_amd import meshdist as md
from psnerf_amd import meshocclude as mo

pytestmark = pytest.mark.gpu
SENTINEL = -77


def dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)                              # (a copy: the cases are read-only)


def same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return np.array_equal(got.view(np.uint64), want.view(np.uint64)) if got.dtype == np.float64 else np.array_equal(got, want)


def guards(R, K, cuda, bits=True):
    n_words = (K + 31) // 32
    return (torch.full((R,), SENTINEL, dtype=torch.int32, device=cuda), torch.full((R,), SENTINEL, dtype=torch.int32, device=cuda),
            torch.full((R,), float('nan'), dtype=torch.float64, device=cuda), torch.full((R, 3), float('nan'), dtype=torch.float64, device=cuda),
            torch.full((R, n_words), SENTINEL, dtype=torch.int32, device=cuda) if bits else None)


def index_of(c, name, cuda):
    """The MeshIndex of a case; for the all-oversize case the same mesh under a grid of small cells with max_span = 1, built by the
    index's own two passes, so that every face lands in the oversize list and the cell lists are empty."""
    if 'every face oversize' not in name:
        return md.MeshIndex(c['v'], c['f'], device=cuda)
    index = md.MeshIndex(c['v'], c['f'], device=cuda, cell=oc.ALL_OVERSIZE_CELL, max_span=1)
    assert index.n_entries == 0 and int(index.cell_start.sum()) == 0 and index.n_over == len(index.over_list) == len(c['f'])
    return index


@pytest.mark.parametrize('name', list(oc.CASES))
def test_device_against_the_definition(cuda, name):
    c = oc.case(name)
    R, K = len(c['points']), len(c['table'])
    index = index_of(c, name, cuda)
    if 'snapped cube' in name:                                   # the case is adversarial only while the vertices sit on the grid's corners
        from tests import raycast_cases as rc
        assert index.cell == rc.SNAP_CELL and index.n == [192, 192, 192]
    if 'two oversize' in name:
        assert index.n_over == 2
    p, n, table = dev(c['points'], cuda), dev(c['normals'], cuda), dev(c['table'], cuda)
    want = c['want']
    n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
    out = guards(R, K, cuda)
    got = index.occlusion(p, n, table, local=c['local'], bias=c['bias'], t_max=c['t_max'], bits=True, n_tests=n_tests, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    hits, visible = got[0].cpu().numpy(), got[1].cpu().numpy()
    cast = int(want[0][~c['dead']].sum() + want[1].sum())
    print('%s: F=%d, %d rows x %d directions, %d cast, %d blocked (host %d), %.1f tests per cast ray' % (
        name, len(c['f']), R, K, cast, int(hits[hits >= 0].sum()), int(want[0][want[0] >= 0].sum()), n_tests.item() / max(cast, 1)))
    assert np.array_equal(hits, want[0]), 'hits differ on %d rows' % int((hits != want[0]).sum())
    assert np.array_equal(visible, want[1])
    assert same_bits(got[2], want[2]), 'ao'
    assert same_bits(got[3], want[3]), 'bent: max difference %g' % np.nanmax(np.abs(got[3].cpu().numpy() - want[3]))
    assert same_bits(got[4], want[4]), 'words'
    assert c['dead'].sum() == (hits == -1).sum() and (R < 63 or c['dead'].sum() == 5)
    # without the bits: the same four, no words; and through the public function on device tensors
    plain = index.occlusion(p, n, table, local=c['local'], bias=c['bias'], t_max=c['t_max'], out=guards(R, K, cuda, bits=False))
    assert plain[4] is None and all(torch.equal(a, b) or same_bits(a, b.cpu().numpy()) for a, b in zip(plain[:4], got[:4]))
    public = mo.occlusion_rows(index, p, n, table, local=c['local'], bias=c['bias'], t_max=c['t_max'], bits=True)
    assert all(x.is_cuda for x in public) and all(same_bits(a, b) for a, b in zip(public, want))
    # two runs, the second on an index built again (its lists may come out in another order), give the same bits
    again = index_of(c, name, cuda).occlusion(p.clone(), n.clone(), table.clone(), local=c['local'], bias=c['bias'], t_max=c['t_max'], bits=True)
    assert all(same_bits(a, b.cpu().numpy()) for a, b in zip(again, got))
    assert cast == 0 or int(n_tests.item()) > 0


@pytest.mark.parametrize('name', ['icosphere, R 257, K 64', 'marching cubes, R 63, K 31, world', 'snapped cube, R 257, K 32, no bias'])
def test_against_materialised_rays(cuda, name):
    """The same rays written out and handed to MeshIndex.ray_cast(any_hit=True), the only route there was: the same blocked counts, and
    the fused kernel makes no more ray-triangle tests than psn_ray_cast does on them (it is the same walk)."""
    from psnerf_amd import hip
    c = oc.case(name)
    R, K = len(c['points']), len(c['table'])
    index = md.MeshIndex(c['v'], c['f'], device=cuda)
    o, d, cast = oc.rays_of(c)
    keep = cast.reshape(-1)
    od, dd = dev(o[keep], cuda), dev(d[keep], cuda)
    hit = index.ray_cast(od, dd, 0.0, c['t_max'], any_hit=True)[3]
    blocked = np.zeros(R * K, dtype=bool)
    blocked[keep] = hit.cpu().numpy()
    n_fused = torch.zeros(1, dtype=torch.int64, device=cuda)
    n_rays = torch.zeros(1, dtype=torch.int64, device=cuda)
    hits = index.occlusion(dev(c['points'], cuda), dev(c['normals'], cuda), dev(c['table'], cuda), local=c['local'], bias=c['bias'], t_max=c['t_max'],
                           n_tests=n_fused)[0].cpu().numpy()
    hip.ray_cast(index.index, od, dd, 0.0, c['t_max'], any_hit=True, n_tests=n_rays)
    print('%s: %d rays, %d blocked; tests: fused %d, materialised %d' % (name, int(keep.sum()), int(blocked.sum()), n_fused.item(), n_rays.item()))
    assert np.array_equal(hits[~c['dead']], blocked.reshape(R, K).sum(axis=1)[~c['dead']])
    assert 0 < int(n_fused.item()) <= int(n_rays.item())


@pytest.mark.parametrize('name', ['icosphere(1)', 'a tetrahedron', 'zero-area faces'])
def test_bake_occlusion_on_the_device(cuda, name):
    """bake_occlusion at T = 64 on a mesh of tests/bake_cases.py: the device bake, in one chunk and in several, equals the host bake bit
    for bit -- every texel of both maps, the fill included."""
    from psnerf_amd import ops
    v, f, vn = bc.meshes()[name]
    mesh = (v, f) if vn is None else (v, f, vn)
    K = 16
    host = mb.bake_occlusion(mesh, size=64, K=K, fill=0.25)
    ops.reset_hits()
    with ops.strict():
        d_mesh = tuple(dev(x, cuda) for x in mesh)
        one = mb.bake_occlusion(d_mesh, size=64, K=K, fill=0.25)
        parts = mb.bake_occlusion(mesh, atlas=host['atlas'], K=K, fill=0.25, chunk_faces=max(1, len(f) // 3), device=cuda)
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    for baked in (one, parts):
        assert baked['occlusion'].is_cuda and baked['occlusion'].dtype == torch.float32 and baked['bent'].shape == (64, 64, 3)
        for key in ('occlusion', 'bent'):
            got, want = baked[key].cpu().numpy(), host[key]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), '%s: %d texels differ' % (key, int((got != want).sum()))
    owned = host['atlas'].owner()[0] >= 0
    print('%s: ao over the owned texels %.3f .. %.3f' % (name, host['occlusion'][owned].min(), host['occlusion'][owned].max()))


def test_vertex_occlusion_on_the_device(cuda):
    """vertex_occlusion of icosphere(2) with inward normals and short rays (so that some directions are blocked and some are not):
    device == host, and device tensors come back."""
    from tests import raycast_cases as rc
    v, f = rc.icosphere(2)
    vn = -mo.area_weighted_normals(v, f)
    host = mo.vertex_occlusion((v, f), vertex_normals=vn, K=16, t_max=0.3, bits=True)
    got = mo.vertex_occlusion((v, f), vertex_normals=vn, K=16, t_max=0.3, bits=True, device=cuda)
    assert all(x.is_cuda for x in got) and got[0].shape == (len(v),) and 0 < int(host[0].sum()) < 16 * len(v)
    assert all(same_bits(a, b) for a, b in zip(got, host))
    on_device = mo.vertex_occlusion((dev(v, cuda), dev(f, cuda), dev(vn, cuda)), K=16, t_max=0.3, bits=True)
    assert all(same_bits(a, b) for a, b in zip(on_device, host))


def test_c_abi_errors(cuda):
    from psnerf_amd import hip
    c = oc.case('icosphere, one row, one direction')
    index = md.MeshIndex(c['v'], c['f'], device=cuda)
    p = torch.zeros(10, 3, dtype=torch.float64, device=cuda)
    n = torch.ones(10, 3, dtype=torch.float64, device=cuda)
    table = lambda K: dev(mo.hemisphere_table(K) if K else np.zeros((0, 3)), cuda)
    call = lambda p, n, t, **kw: hip.occlusion_rows(index.index, p, n, t, **kw)
    assert bool((call(p, n, table(1024))[0] == 1024).all())                  # rows at the centre of the sphere: everything is blocked
    wide = torch.ones(10, 6, dtype=torch.float64, device=cuda)
    for bad in (lambda: call(p, n, table(0)), lambda: call(p, n, table(1025)), lambda: call(p.cpu(), n, table(4)), lambda: call(p, n.float(), table(4)),
                lambda: call(p[:5], n, table(4)), lambda: call(wide[:, ::2], n, table(4)), lambda: call(p, n, table(4), bias=float('inf')),
                lambda: call(p, n, table(4), t_max=-1.0), lambda: call(p, n, table(4), t_max=float('nan')),
                lambda: call(p, n, table(4), out=guards(9, 4, cuda, bits=False))):
        with pytest.raises(RuntimeError, match='occlusion_rows'):
            bad()
    hits, visible, ao, bent, words = call(p[:0], n[:0], table(33), bits=True)
    assert hits.shape == (0,) and ao.shape == (0,) and bent.shape == (0, 3) and words.shape == (0, 2) and hits.is_cuda
    # null pointers and a bad mode, which the wrapper cannot produce: the entry point itself
    out = guards(10, 4, cuda)
    t4 = table(4)
    args = collections.OrderedDict([('index', ctypes.byref(index.index)), ('points', p.data_ptr()), ('normals', n.data_ptr()), ('n_rows', 10),
                                    ('table', t4.data_ptr()), ('n_dirs', 4), ('mode', hip.OCC_LOCAL), ('bias', 0.0), ('t_max', float('inf')),
                                    ('hits', out[0].data_ptr()), ('visible', out[1].data_ptr()), ('ao', out[2].data_ptr()),
                                    ('bent', out[3].data_ptr()), ('words', out[4].data_ptr()), ('n_tests', None), ('stream', None)])
    assert hip._lib.psn_occlusion_rows(*args.values()) == 0
    torch.cuda.synchronize()
    assert bool((out[0] == 4).all())
    for key, value in (('index', None), ('vertices', None), ('faces', None), ('cell_start', None), ('points', None), ('normals', None),
                       ('table', None), ('hits', None), ('visible', None), ('ao', None), ('bent', None), ('mode', 2), ('mode', -1), ('n_dirs', 0),
                       ('n_dirs', 1025), ('n_rows', -1)):
        broken = collections.OrderedDict(args)
        if key in broken:
            broken[key] = value
        else:                                                            # a field of the index: one changed in a copy of the struct
            ix = hip.PsnMeshIndex.from_buffer_copy(index.index)
            setattr(ix, key, value)
            broken['index'] = ctypes.byref(ix)
        assert hip._lib.psn_occlusion_rows(*broken.values()) == hip.E_ARG, '%s = %r' % (key, value)
        assert b'occlusion_rows' in hip._lib.psn_last_error()
