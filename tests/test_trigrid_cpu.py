"""The triangle grid's host definition (psnerf_amd.meshdist.host_tri_grid) against meshes constructed in integer cell units, and the
pure grid choice (grid_shape) against what MeshIndex has always arrived at.  The device index is compared with the same definition
in tests/test_trigrid_gpu.py; the cases are tests/trigrid_cases.py."""
import numpy as np
import pytest

from tests import raycast_cases as rc
from tests import trigrid_cases as tc
from psnerf_amd import meshdist as md


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_pinned_counts_and_list_structure(name):
    """What the definition counted on each case, and the facts that tie its lists together: a triangle is in a cell's list iff the
    cell is in its range and it is not oversize; the counts sum to n_entries; cell_start is their exclusive scan with the total
    appended; no id is both listed and oversize; ids ascend within a cell."""
    c, d = tc.case(name), tc.definition(name)
    n, F = c['n'], len(c['faces'])
    cells = n[0] * n[1] * n[2]
    counted = (F, n, len(d['over']), len(d['list']), int((d['cell_count'] > 0).sum()))
    print('%s: %r, cell %r' % (name, counted, c['cell']))
    assert counted == tc.CASES[name]
    assert d['cell_count'].shape == (cells,) and d['cell_start'].shape == (cells + 1,) and d['cell_count'].dtype == np.int64
    assert int(d['cell_count'].sum()) == len(d['list']) == int(d['cell_start'][-1])
    assert d['cell_start'][0] == 0 and np.array_equal(np.diff(d['cell_start']), d['cell_count'])
    assert np.array_equal(d['cell_start'][:-1], np.cumsum(d['cell_count']) - d['cell_count'])
    assert np.array_equal(d['over'], np.nonzero(d['span'] > c['max_span'])[0]) and not np.intersect1d(d['over'], d['list']).size
    assert (d['c0'] >= 0).all() and (d['c0'] <= d['c1']).all() and (d['c1'] <= np.asarray(n) - 1).all()
    assert np.array_equal(d['span'], np.prod(d['c1'] - d['c0'] + 1, axis=1))
    # membership, from the other side: every (cell, id) pair of the lists, decoded, against the ranges
    cell_of = np.repeat(np.arange(cells), d['cell_count'])
    ids = d['list']
    xyz = np.stack([cell_of // (n[1] * n[2]), cell_of // n[2] % n[1], cell_of % n[2]], axis=1)
    assert ((xyz >= d['c0'][ids]) & (xyz <= d['c1'][ids])).all() and (d['span'][ids] <= c['max_span']).all()
    listed = d['span'] <= c['max_span']
    assert np.array_equal(np.bincount(ids, minlength=F), np.where(listed, d['span'], 0))      # every cell of the range, each once
    pair = cell_of * F + ids
    assert (np.diff(pair) > 0).all()                                                          # by cell, ascending ids, no pair twice


@pytest.mark.parametrize('name', ['lattice soup', 'oversize by lane', 'oversize by lane, none oversize'])
def test_definition_against_construction(name):
    """c0, c1 and span equal the integer construction, which never went through a floor: interior corners, corners snapped onto grid
    corners (a snapped upper corner belongs to the upper cell) and corners at hi (clamped into n - 1)."""
    c, d = tc.case(name), tc.definition(name)
    c0, c1, span = c['construction']
    assert np.array_equal(d['c0'], c0) and np.array_equal(d['c1'], c1) and np.array_equal(d['span'], span)
    assert c['lo'] == [tc.SOUP_LO] * 3 and c['hi'] == [-tc.SOUP_LO] * 3 and c['cell'] == tc.SOUP_CELL and c['n'] == [tc.SOUP_N] * 3
    q = (c['vertices'] - tc.SOUP_LO) / tc.SOUP_CELL                # in cells: what the cases promise about where corners sit
    assert (q == np.round(q)).any() and (q == tc.SOUP_N).any() and (q != np.round(q)).any()
    if name == 'lattice soup':
        shapes = sorted(set(map(tuple, (c1 - c0 + 1)[:-1].tolist())))
        assert shapes == sorted(tc.SOUP_SHAPES) and tuple((c1 - c0 + 1)[-1]) == (16, 16, 16)
        assert sorted(set(span[:-1].tolist())) == [1, 8, 9]                                   # both sides of max_span = 8
        per_wave = np.bincount(d['over'] // 64, minlength=11)
        assert len(per_wave) == 11 and per_wave.min() >= 20 and per_wave.max() <= 40          # sparse in every wave
    elif name == 'oversize by lane':
        assert d['over'].tolist() == sorted(tc.LANE_OVERSIZE) and len(c['faces']) % 64 != 0
        lanes = dict((w, (d['over'][d['over'] // 64 == w] % 64).tolist()) for w in range(11))
        assert lanes[0] == [0, 63] and lanes[1] == list(range(64)) and lanes[2] == [] and lanes[3] == [31, 32] and lanes[4] == [0]
        assert lanes[10] == [(tc.LANE_FACES - 1) % 64] and all(lanes[w] == [] for w in range(5, 10))
    else:
        assert d['over'].size == 0 and d['span'].max() == tc.SOUP_N ** 3


def test_small_grids():
    """One triangle listed and oversize, one layer of cells, one cell."""
    c, d = tc.case('one triangle'), tc.definition('one triangle')
    assert d['span'].tolist() == [27] and d['list'].tolist() == [0] * 27 and (d['cell_count'] == 1).all()
    d = tc.definition('one triangle, oversize')
    assert d['over'].tolist() == [0] and d['list'].size == 0 and not d['cell_count'].any() and not d['cell_start'].any()
    assert tc.case('flat box')['n'][2] == 1 and tc.case('flat box')['lo'][2] == tc.case('flat box')['hi'][2]
    c, d = tc.case('mesh in one point'), tc.definition('mesh in one point')
    assert c['cell'] == 1.0 and c['n'] == [1, 1, 1] and c['lo'] == c['hi'] and d['list'].tolist() == [0, 1, 2, 3]
    c = tc.case('cell 0.1')
    k = (c['vertices'] - np.asarray(c['lo'])) / 0.1
    assert np.abs(k - np.round(k)).max() < 1e-9 and (k != np.round(k)).any()                  # on the lattice, to rounding only


def _suite_meshes():
    out = {'snapped cube': rc.snapped_cube(6)[:2], 'marching cubes': rc.mc_mesh(), 'icosphere(2)': rc.icosphere(2)}
    out.update(rc.awkward_meshes())
    return out


def test_grid_shape():
    """grid_shape is MeshIndex's former inline choice: the formulas written out here once more, on the suite's meshes; n >= 1; a
    zero extent gives n = 1; one point gives cell = 1; lo + n cell >= hi whenever no axis was clamped; a truncated grid is seen."""
    for name, (v, f) in _suite_meshes().items():
        lo, hi = v.min(0).tolist(), v.max(0).tolist()
        edge = tc.mean_edge(v, f)
        cell, n = md.grid_shape(lo, hi, edge)
        extent = [hi[i] - lo[i] for i in range(3)]
        want = max(edge, max(extent) / 192)
        assert cell == want and n == [int(min(192, max(1, np.ceil(e / want)))) for e in extent], name
        assert all(isinstance(k, int) and 1 <= k <= md.CELLS_PER_AXIS for k in n) and not md.grid_truncated(lo, hi, cell, n), name
        if name in tc.CASES:
            assert n == tc.CASES[name][1], name
        for given in (0.37 * cell, 3.0 * cell, max(extent) / 191.5):
            c2, n2 = md.grid_shape(lo, hi, edge, given)
            assert c2 == given and all(1 <= k <= 192 for k in n2)
            if max(n2) < 192:
                assert all(lo[i] + n2[i] * c2 >= hi[i] for i in range(3)) and not md.grid_truncated(lo, hi, c2, n2), (name, given)
    v, f = rc.snapped_cube(6)[:2]
    assert md.grid_shape(v.min(0).tolist(), v.max(0).tolist(), tc.mean_edge(v, f)) == (rc.SNAP_CELL, [192] * 3)
    flat = rc.awkward_meshes()['flat bounding box'][0]
    assert md.grid_shape(flat.min(0).tolist(), flat.max(0).tolist(), 0.1)[1][2] == 1
    assert md.grid_shape([0.3, -0.6, 0.9], [0.3, -0.6, 0.9], 0.0) == (1.0, [1, 1, 1])
    assert md.grid_shape([0.3, -0.6, 0.9], [0.3, -0.6, 0.9], float('nan')) == (1.0, [1, 1, 1])
    assert md.grid_shape([0.0] * 3, [1.0, 0.0, 2.0], float('nan')) == (2.0 / 192, [96, 1, 192])
    # random boxes and cells: whenever no axis reaches the clamp the grid covers the box
    g = np.random.RandomState(0)
    for _ in range(2000):
        lo = (g.standard_normal(3) * 3.0).tolist()
        hi = [lo[i] + float(g.rand() ** 3) * 5.0 for i in range(3)]
        cell, n = md.grid_shape(lo, hi, float(g.rand() * 0.3) + 1e-3, None if g.rand() < 0.5 else float(g.rand() * 0.2) + 1e-3)
        assert all(1 <= k <= 192 for k in n)
        if max(n) < 192:
            assert not md.grid_truncated(lo, hi, cell, n), (lo, hi, cell, n)
    c = tc.case('truncated grid')
    assert c['n'] == [192] * 3 and c['cell'] == max(c['hi'][i] - c['lo'][i] for i in range(3)) / 400.0 and md.grid_truncated(c['lo'], c['hi'], c['cell'], c['n'])
    assert all(c['lo'][i] + 192 * c['cell'] < c['hi'][i] for i in range(3))
    d = tc.definition('truncated grid')
    beyond = (c['vertices'] > np.asarray(c['lo']) + 192 * c['cell']).all(axis=1)              # vertices past the grid on every axis
    assert beyond.any() and (d['c1'].max(axis=0) == 191).all() and d['cell_count'][-1] > 0    # ... are held by the last cell
