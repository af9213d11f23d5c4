"""Crossing counts on the GPU (csrc/meshinside.hip through MeshIndex.crossings / contains) against the float64 numpy definition
meshdist.host_crossings, on every mesh x point set of tests/inside_cases.py and every axis.

What is demanded, and why.  ``above``, ``below`` and ``on`` are integers and must be EQUAL on every point: the test is a fixed
sequence of correctly rounded float64 + - x / and comparisons, the same on both sides, with contraction off -- and the definition
knows no grid, so the device's walk may neither lose a triangle nor count one twice.  A mismatch is a finding about the walk or the
once-only rule, not a tolerance to widen.  The adversarial pairs are the point: points exactly on the grid's column boundaries (and
within half a margin of them) under a box whose vertices sit on the grid's corners, points under the mesh's own vertices and edge
midpoints, the vertices themselves, the oversize list, the flat box, the one-triangle mesh."""
import ctypes

import numpy as np
import pytest
import torch

from tests import inside_cases as ic
from tests import raycast_cases as rc
from psnerf_amd import meshdist as md

pytestmark = pytest.mark.gpu
MESHES = ['snapped box', 'marching-cubes sphere', 'icosphere(2)', 'hemisphere', 'nested spheres', 'two oversize triangles',
          'degenerate triangles', 'a single triangle', 'flat bounding box']
_REFERENCE = {}


def mesh_case(name):
    """-> (vertices, faces, focus or None, points per set): the sets of one axis hold 7.2 x that many points, and over the three axes
    points x faces stays at or below 2e7 for the brute-force definition."""
    if name == 'snapped box':
        v, f, n_cube = rc.snapped_cube(6)
        return v, f, (v[:n_cube].min(0), v[:n_cube].max(0)), 1500
    if name == 'marching-cubes sphere':
        return ic.mc_sphere()[:2] + (None, 1000)
    if name == 'icosphere(2)':
        return rc.icosphere(2) + (None, 1500)
    if name == 'hemisphere':
        return ic.hemisphere(2) + (None, 1500)
    if name == 'nested spheres':
        return ic.nested(2, 0.5) + (None, 1400)
    return rc.awkward_meshes()[name] + (None, 1500 if name == 'a single triangle' else 600)


def reference(name, axis, index):
    """The point sets of a mesh and an axis (laid along the grid ``index`` reports) with the definition's answer, computed once."""
    if (name, axis) not in _REFERENCE:
        v, f, focus, count = mesh_case(name)
        sets = ic.point_sets(v, f, index.lo, index.cell, index.n, axis, count, seed=len(name) + axis, focus=focus)
        _REFERENCE[(name, axis)] = dict((s, (p,) + md.host_crossings(v, f, p, axis)) for s, p in sets.items())
    return _REFERENCE[(name, axis)]


def equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('name', MESHES)
def test_device_against_the_definition(cuda, name):
    from psnerf_amd import hip
    v, f, focus, count = mesh_case(name)
    index = md.MeshIndex(v, f, device=cuda)
    again = md.MeshIndex(v, f, device=cuda)                      # (its lists may come out in another order)
    if name == 'snapped box':                                    # the case is adversarial only while the vertices sit on the grid's corners
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
    total_q = 0
    for axis in range(3):
        for sname, (p, h_above, h_below, h_on) in reference(name, axis, index).items():
            what = '%s, axis %d, %s' % (name, axis, sname)
            total_q += len(p)
            pd = torch.from_numpy(p).to(cuda)
            n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
            out = index.crossings(pd, axis, n_tests=n_tests)
            above, below, on = (x.cpu().numpy() for x in out)
            n = int(n_tests.item())
            print('%s: F=%d Q=%d, above / below / on differ on %d / %d / %d points; inside %d, open %d, on > 0: %d; %.1f tests per point' % (
                what, len(f), len(p), int((above != h_above).sum()), int((below != h_below).sum()), int((on != h_on).sum()),
                int((h_above & 1).sum()), int(((h_above + h_below + h_on) & 1).sum()), int((h_on > 0).sum()), n / len(p)))
            assert above.dtype == np.int32 and below.dtype == np.int32 and on.dtype == np.int32
            assert np.array_equal(above, h_above), what + ': above differs on %d points' % int((above != h_above).sum())
            assert np.array_equal(below, h_below), what + ': below differs on %d points' % int((below != h_below).sum())
            assert np.array_equal(on, h_on), what + ': on differs on %d points' % int((on != h_on).sum())
            finite = np.isfinite(p).all(axis=1)
            kx, ky = (axis + 1) % 3, (axis + 2) % 3
            walked = finite & (p[:, kx] >= v[:, kx].min()) & (p[:, kx] <= v[:, kx].max()) & (p[:, ky] >= v[:, ky].min()) & (p[:, ky] <= v[:, ky].max())
            assert n <= len(p) * len(f) and (n > 0 or not (h_above + h_below + h_on).any()), what
            assert n >= index.n_over * int(walked.sum()), what
            # without below: the same above and on
            half = index.crossings(pd, axis, below=False)
            assert half[1] is None and torch.equal(half[0], out[0]) and torch.equal(half[2], out[2]), what + ': below=False changes above / on'
            # a second run on a rebuilt index; the order of the work: a random permutation, and none
            assert equal(out, again.crossings(pd.clone(), axis)), what + ': two runs differ'
            raw = lambda order: hip.mesh_crossings(index.index, pd, axis=axis, order=order)
            assert equal(out, raw(None)) and equal(out, raw(torch.randperm(len(p), generator=g).to(cuda))), what + ': the order changes the result'
            if sname == 'uniform, box + 10 %':
                assert torch.equal(index.contains(pd, axis), out[0] % 2 == 1)
                if name == 'marching-cubes sphere':              # that the grid saves tests is a condition, not a timing
                    assert 0 < n < len(p) * len(f) / 10, what
                if name in ('marching-cubes sphere', 'icosphere(2)', 'nested spheres', 'snapped box'):
                    assert 0 < int((h_above & 1).sum()) < len(p)
    assert total_q * len(f) <= 2e7


def test_lattice_queries_and_vote_on_the_device(cuda):
    """The sphere's own padded lattice (every line through vertices): inside == the field's sign on all three axes and for the vote;
    on the hemisphere contains(vote=True) is the host's."""
    v, f, field, lattice = ic.mc_sphere()
    index = md.MeshIndex(v, f, device=cuda)
    pd = torch.from_numpy(lattice).to(cuda)
    want = torch.from_numpy(field > 0.0).to(cuda)
    for axis in range(3):
        above, below, on = index.crossings(pd, axis)
        assert torch.equal(index.contains(pd, axis), want) and not bool(((above + below + on) & 1).any())
    assert torch.equal(index.contains(pd, vote=True), want)
    hv, hf = ic.hemisphere(2)
    p = (np.random.RandomState(3).random_sample((3000, 3)) - 0.5) * 2.2
    host = md._HostMesh(hv, hf)
    dome = md.MeshIndex(hv, hf, device=cuda)
    single, vote = dome.contains(torch.from_numpy(p).to(cuda)), dome.contains(torch.from_numpy(p).to(cuda), vote=True)
    assert single.dtype == torch.bool and np.array_equal(single.cpu().numpy(), host.contains(p))
    assert np.array_equal(vote.cpu().numpy(), host.contains(p, vote=True)) and not torch.equal(single, vote)


def test_c_abi_errors(cuda):
    from psnerf_amd import hip
    v, f = rc.icosphere(2)
    index = md.MeshIndex(v, f, device=cuda)
    p = torch.zeros(10, 3, dtype=torch.float64, device=cuda)
    count = lambda p, **kw: hip.mesh_crossings(index.index, p, **kw)
    above, below, on = count(p)
    assert above.tolist() == [1] * 10 and below.tolist() == [1] * 10 and on.tolist() == [0] * 10
    wide = torch.ones(10, 6, dtype=torch.float64, device=cuda)
    for bad in (lambda: count(p.cpu()), lambda: count(p.float()), lambda: count(wide[:, :3]), lambda: count(wide), lambda: count(p, axis=3),
                lambda: count(p, axis=-1)):
        with pytest.raises(RuntimeError, match='mesh_crossings'):
            bad()
    with pytest.raises(ValueError):
        index.crossings(p, axis=3)
    with pytest.raises(RuntimeError):
        index.crossings(p.cpu())
    above, below, on = count(p[:0])
    assert above.shape == (0,) and below.shape == (0,) and on.shape == (0,) and above.is_cuda and above.dtype == torch.int32
    # the C ABI itself: null pointers, axis 3, Q = 0
    out = torch.full((10,), -7, dtype=torch.int32, device=cuda)
    def struct(**fields):                                        # the index with no oversize list, and one field changed in the copy
        ix = hip.PsnMeshIndex.from_buffer_copy(index.index)
        for k, value in dict({'over_list': None, 'n_over': 0}, **fields).items():
            setattr(ix, k, value)
        return ctypes.byref(ix)

    def call(**kw):
        ix = struct(**{k: kw.pop(k) for k in list(kw) if k in dict(hip.PsnMeshIndex._fields_)})
        return hip._lib.psn_mesh_crossings(*[kw.get(k, d) for k, d in (('index', ix), ('points', p.data_ptr()), ('order', None), ('n_points', 10),
                                                                        ('axis', 2), ('above', out.data_ptr()), ('below', None), ('on', None),
                                                                        ('n_tests', None), ('stream', None))])
    assert index.index.n_faces == len(f)
    for kw in ({'index': None}, {'vertices': None}, {'faces': None}, {'cell_start': None}, {'list': None}, {'points': None}, {'above': None},
               {'axis': 3}, {'axis': -1}, {'n_points': -1}, {'n_faces': 0}, {'n_over': 1}):
        assert call(**kw) == hip.E_ARG, kw                       # noqa: F821 (from the header)
        assert b'mesh_crossings' in hip._lib.psn_last_error()
    torch.cuda.synchronize()
    assert out.tolist() == [-7] * 10
    assert call(n_points=0, points=None, above=None) == hip.OK and out.tolist() == [-7] * 10
    assert call() == hip.OK and out.tolist() == [1] * 10
