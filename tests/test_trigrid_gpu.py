"""The triangle grid that csrc/meshdist.hip builds (psn_tri_grid_count -> torch.cumsum -> psn_tri_grid_fill through MeshIndex)
against its host definition psnerf_amd.meshdist.host_tri_grid, on the cases of tests/trigrid_cases.py.

Every comparison of the index is EQUAL: the cells are integers, and they come from float64 operations that are correctly rounded on
both sides with contraction off (a subtraction, a product, a floor), so there is no tolerance to choose.  The order of the ids within
a cell's list and within the oversize list is not defined (atomics); both are sorted before they are compared.  The queries on the
new grids are held to the gates of the tests they come from (tests/test_chamfer_gpu.py, tests/test_raycast_gpu.py,
tests/test_inside_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import trigrid_cases as tc
from tests.test_chamfer_gpu import GATE, check_against_host, diagonal
from psnerf_amd import meshdist as md

pytestmark = pytest.mark.gpu
_INDEX = {}


def grid_args(c):
    return dict(cell=c['cell_arg'], max_span=c['max_span'])


def build(cuda, name, fresh=False):
    """The MeshIndex of a case (built once unless ``fresh``), checked to lie in the grid the case states, and the definition on
    exactly that grid."""
    c = tc.case(name)
    if fresh or name not in _INDEX:
        index = md.MeshIndex(c['vertices'], c['faces'], device=cuda, **grid_args(c))
        if fresh:
            return index
        _INDEX[name] = index
    index = _INDEX[name]
    assert index.lo == c['lo'] and index.hi == c['hi'] and index.n == c['n'] == tc.CASES[name][1], name
    if name in tc.EXPLICIT_CELL:
        assert index.cell == c['cell'], name
    assert abs(index.cell - c['cell']) <= 1e-14 * c['cell'], name
    return c, index, tc.definition(name, index.cell)


def sorted_lists(cell_start, lst, over_list, F):
    """(list sorted within each cell, oversize list sorted) as int64 numpy; cell_start must already be known to be right."""
    cs = cell_start.cpu().numpy().astype(np.int64)
    ids = lst.cpu().numpy().astype(np.int64)[:cs[-1]]
    cell_of = np.repeat(np.arange(len(cs) - 1), np.diff(cs))
    return ids[np.argsort(cell_of * F + ids, kind='stable')], np.sort(over_list.cpu().numpy().astype(np.int64))


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_index_against_the_definition(cuda, name):
    c, index, d = build(cuda, name)
    F = len(c['faces'])
    counted = (F, index.n, index.n_over, index.n_entries, int((index.cell_start[1:] > index.cell_start[:-1]).sum()))
    print('%s: device %r, pinned %r, cell %r' % (name, counted, tc.CASES[name], index.cell))
    assert index.cell_start.dtype == torch.int32 and index.list.dtype == torch.int32 and index.over_list.dtype == torch.int32
    assert np.array_equal(index.cell_start.cpu().numpy().astype(np.int64), d['cell_start']), name + ': cell_start'
    assert index.n_entries == len(d['list']) and index.n_over == len(d['over']), name
    assert index.over_list.numel() == index.n_over and index.list.numel() == max(index.n_entries, 1)
    lst, over = sorted_lists(index.cell_start, index.list, index.over_list, F)
    assert lst.size == 0 or (lst.min() >= 0 and lst.max() <= F - 1), name + ': a list entry is no triangle id'
    assert np.array_equal(lst, d['list']), name + ': cell lists'
    assert np.array_equal(over, d['over']), name + ': oversize list'
    if name in tc.EXPLICIT_CELL:
        assert counted == tc.CASES[name], name
    if index.n_entries == 0:                                     # the placeholder list, and the n_over == F rule of md_check_index
        assert index.n_over == F and index.list.tolist() == [0]
    again = build(cuda, name, fresh=True)
    assert torch.equal(again.cell_start, index.cell_start) and (again.n_over, again.n_entries) == (index.n_over, index.n_entries)
    lst2, over2 = sorted_lists(again.cell_start, again.list, again.over_list, F)
    assert np.array_equal(lst2, lst) and np.array_equal(over2, over), name + ': two builds differ'


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_raw_entries_on_dirty_buffers(cuda, name):
    """psn_tri_grid_count and psn_tri_grid_fill on buffers that hold other numbers: cell_count is zeroed there, n_over is set there,
    over_list is written up to n_over and no further, the cursor ends as the inclusive scan, every list entry is written."""
    from psnerf_amd import hip
    c, index, d = build(cuda, name)
    v, f = index.vertices, index.faces
    F, cells = len(c['faces']), len(d['cell_count'])
    grid = hip.tri_grid(index.lo, index.hi, index.cell, index.n, c['max_span'])
    cell_count = torch.full((cells,), 7, dtype=torch.int32, device=cuda)
    over_list = torch.full((F,), -9, dtype=torch.int32, device=cuda)
    n_over = torch.full((1,), 12345, dtype=torch.int64, device=cuda)
    for run in range(2):                                         # the second call meets the first one's results
        out = hip.tri_grid_count(grid, v, f, n_over, out=(cell_count, over_list))
        assert out[0] is cell_count and out[1] is over_list
        assert np.array_equal(cell_count.cpu().numpy().astype(np.int64), d['cell_count']), '%s: counts, call %d' % (name, run)
        k = int(n_over.item())
        assert k == len(d['over']), '%s: n_over, call %d' % (name, run)
        assert np.array_equal(np.sort(over_list[:k].cpu().numpy().astype(np.int64)), d['over']), '%s: oversize list, call %d' % (name, run)
        assert bool((over_list[k:] == -9).all()), '%s: over_list written beyond n_over, call %d' % (name, run)
    n_entries = len(d['list'])
    cursor = torch.from_numpy(d['cell_start'][:-1].astype(np.int32)).to(cuda)
    guard = torch.full((n_entries,), -5, dtype=torch.int32, device=cuda)
    lst = hip.tri_grid_fill(grid, v, f, cursor, n_entries, out=guard)
    assert lst is guard
    assert np.array_equal(cursor.cpu().numpy().astype(np.int64), d['cell_start'][1:]), name + ': the cursor is not the inclusive scan'
    assert not bool((lst == -5).any()), name + ': a list entry was never written'
    cell_start = torch.from_numpy(d['cell_start'].astype(np.int32))
    assert np.array_equal(sorted_lists(cell_start, lst, over_list[:k], F)[0], d['list']), name + ': cell lists'
    with pytest.raises(RuntimeError, match='out must be'):
        hip.tri_grid_count(grid, v, f, n_over, out=(cell_count[:-1], over_list))
    with pytest.raises(RuntimeError, match='out must be'):
        hip.tri_grid_fill(grid, v, f, cursor, n_entries, out=guard.to(torch.int64))


def same(a, b):
    return all(torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)) if x.dtype.is_floating_point else torch.equal(x, y)
               for x, y in zip(a, b))


@pytest.mark.parametrize('name', tc.QUERY_CASES)
def test_queries_on_the_new_grids(cuda, name):
    """Closest point, ray casting and crossings through these grids against their brute-force definitions: points and origins in and
    around the box, on cell boundaries, at lo and hi, far outside."""
    c, index, d = build(cuda, name)
    v, f = c['vertices'], c['faces']
    diag = diagonal(v)
    assert index.n_over > 0 and index.n_entries > 0
    # closest point
    check_against_host(cuda, v, f, tc.query_points(c, 500, 1), name + ', closest point', **grid_args(c))
    # rays
    o, dr = tc.query_rays(c, 500, 2)
    h_t, h_tri, h_bary, h_hit = md.host_ray_cast(v, f, o, dr)
    od, dd = torch.from_numpy(o).to(cuda), torch.from_numpy(dr).to(cuda)
    out = index.ray_cast(od, dd)
    assert same(out, build(cuda, name, fresh=True).ray_cast(od.clone(), dd.clone())), name + ': two ray casts differ'
    any_hit = index.ray_cast(od, dd, any_hit=True)[3].cpu().numpy()
    t, tri, bary, hit = (x.cpu().numpy() for x in out)
    print('%s: %d rays, %d hit (host %d), ids equal %d' % (name, len(o), int(hit.sum()), int(h_hit.sum()), int((tri == h_tri).sum())))
    assert 0 < h_hit.sum() < len(o)
    assert np.array_equal(hit, h_hit), name + ': hit differs on %d rays' % int((hit != h_hit).sum())
    assert np.array_equal(any_hit, h_hit), name + ': any-hit differs on %d rays' % int((any_hit != h_hit).sum())
    assert np.array_equal(tri >= 0, hit) and tri.max() < len(f) and (t[~hit] == np.inf).all() and np.isnan(bary[~hit]).all()
    r_t, r_bary, r_ok = md.host_ray_triangle(v, f, o, dr, tri)
    err = float(np.abs(t[hit] - h_t[hit]).max())
    err_tri, err_bary = float(np.abs(r_t[hit] - t[hit]).max()), float(np.abs(r_bary[hit] - bary[hit]).max())
    print('    max |t - t_host| = %.3e, to the returned triangle %.3e, barycentrics %.3e (gate %.3e)' % (err, err_tri, err_bary, GATE * diag))
    assert r_ok[hit].all() and err <= GATE * diag and err_tri <= GATE * diag and err_bary <= GATE, name
    # crossings
    p = tc.query_points(c, 500, 3)
    pd = torch.from_numpy(p).to(cuda)
    for axis in range(3):
        h = md.host_crossings(v, f, p, axis)
        got = index.crossings(pd, axis)
        assert h[0].any() and all(x.dtype == torch.int32 for x in got)
        for what, x, y in zip(('above', 'below', 'on'), got, h):
            assert np.array_equal(x.cpu().numpy(), y), '%s, axis %d: %s differs on %d points' % (name, axis, what, int((x.cpu().numpy() != y).sum()))
        half = index.crossings(pd, axis, below=False)
        assert half[1] is None and torch.equal(half[0], got[0]) and torch.equal(half[2], got[2])


@pytest.mark.parametrize('name', tc.QUERY_CASES + ['flat box', 'cell 0.1'])
def test_crossings_counter_is_the_once_only_rule(cuda, name):
    """Points at cell centres, where the margin can not reach a second column: n_tests = the oversize list for every point inside the
    box across the axis, plus the listed triangles whose range across the axis holds the point's column -- all of them with
    ``below``, those that reach the point's cell or above without.  Each triangle once, however many cells of the column list it;
    this does not look at what the test then accepts."""
    c, index, d = build(cuda, name)
    lo, hi = np.asarray(c['lo']), np.asarray(c['hi'])
    listed = d['span'] <= c['max_span']
    c0, c1 = d['c0'][listed], d['c1'][listed]
    for axis in range(3):
        kx, ky = (axis + 1) % 3, (axis + 2) % 3
        p, k = tc.cell_centres(c, 400, 10 + axis, axis)
        in_box = (p[:, kx] >= lo[kx]) & (p[:, kx] <= hi[kx]) & (p[:, ky] >= lo[ky]) & (p[:, ky] <= hi[ky])
        column = ((c0[None, :, kx] <= k[:, None, kx]) & (k[:, None, kx] <= c1[None, :, kx]) &
                  (c0[None, :, ky] <= k[:, None, ky]) & (k[:, None, ky] <= c1[None, :, ky]))             # [Q, listed]
        upward = column & (c1[None, :, axis] >= k[:, None, axis])
        pd = torch.from_numpy(p).to(cuda)
        for below, met in ((True, column), (False, upward)):
            want = int((in_box * (len(d['over']) + met.sum(axis=1))).sum())
            n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
            got = index.crossings(pd, axis, below=below, n_tests=n_tests)
            print('%s, axis %d, below=%s: %d points (%d in the box), %d tests, expected %d' % (name, axis, below, len(p), int(in_box.sum()),
                                                                                              int(n_tests.item()), want))
            assert int(n_tests.item()) == want, '%s, axis %d, below=%s' % (name, axis, below)
            h = md.host_crossings(c['vertices'], c['faces'], p, axis)
            assert np.array_equal(got[0].cpu().numpy(), h[0]) and np.array_equal(got[2].cpu().numpy(), h[2])
        if name in tc.QUERY_CASES:
            assert 0 < in_box.sum() < len(p) and column.any() and (upward != column).any()


@pytest.mark.parametrize('name', tc.QUERY_CASES + ['marching cubes'])
def test_closest_point_counter(cuda, name):
    """Every point tests the oversize list and its home cell's list at the least, and visits no cell twice:
    sum (n_over + |home list|) <= n_tests <= Q (n_over + n_entries), on every grid.

    n_tests <= Q F as well, where a triangle is listed in few cells (max_span 8 in the two lattice cases, the default grid of the
    marching-cubes mesh).  That is no law of this search: it tests a triangle in EVERY visited cell that lists it (only the
    crossings kernel has a once-only rule), so on the truncated grid, where max_span = 4096 lets one triangle into thousands of
    cells of 1 / 200 and a point half a radius from the surface walks a hundred shells of them, 508 points made 14 577 973 tests
    against Q F = 162 560 (measured on an MI355X).  There the two bounds of the
    first sentence are what is asserted."""
    c, index, d = build(cuda, name)
    p = tc.query_points(c, 500, 4)
    home = tc.home_cells(c, p, index.cell)
    cell = (home[:, 0] * c['n'][1] + home[:, 1]) * c['n'][2] + home[:, 2]
    least = int((len(d['over']) + d['cell_count'][cell]).sum())
    most = len(p) * (len(d['over']) + len(d['list']))
    n_tests = torch.zeros(1, dtype=torch.int64, device=cuda)
    index.closest_point(torch.from_numpy(p).to(cuda), n_tests=n_tests)
    n = int(n_tests.item())
    print('%s: %d points, %d tests, at least %d, Q F = %d, Q (n_over + n_entries) = %d' % (name, len(p), n, least, len(p) * len(c['faces']), most))
    assert least <= n <= most, name
    if name != 'truncated grid':
        assert n <= len(p) * len(c['faces']), name
