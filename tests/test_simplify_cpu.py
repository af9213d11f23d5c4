"""The definition of the mesh simplification (psnerf_amd/meshsimplify.py:host_*) on the host: properties that follow from the
definition, the corner gate that tells the quadric minimiser from the centroid, flat regions, the face budget and its bisection,
three wrong formulations shown to fail these same checks, argument errors and degenerate sizes.  The meshes are
tests/simplify_cases.py; the device path is held to this definition bit for bit in tests/test_simplify_gpu.py."""
import math

import numpy as np
import pytest

from psnerf_amd import meshsimplify as ms
from tests.simplify_cases import RUNS, ROTATED_RESOLUTIONS, SLAB_H, case, host_result, run_id


def rotated_triples(faces):
    f = np.asarray(faces)
    first = f.argmin(axis=1)
    rows = np.arange(len(f))
    return np.stack([f[rows, first], f[rows, (first + 1) % 3], f[rows, (first + 2) % 3]], axis=1)


def failed_properties(v, f, out_v, out_f, report, kw):
    """The names of the definition's properties that (out_v, out_f, report) does not have."""
    failed = []
    if len(f) != report['n_faces'] + report['n_faces_degenerate'] + report['n_faces_duplicate'] or report['n_faces'] != len(out_f) \
            or report['n_vertices'] != len(out_v):
        failed.append('counters')
    if len(out_f) and ((out_f[:, 0] == out_f[:, 1]) | (out_f[:, 1] == out_f[:, 2]) | (out_f[:, 0] == out_f[:, 2])).any():
        failed.append('three different vertices')
    if len(np.unique(rotated_triples(out_f), axis=0)) != len(out_f):
        failed.append('a rotated triple twice')
    if not np.array_equal(np.unique(out_f), np.arange(len(out_v))):
        failed.append('every vertex named')
    if len(out_f) == 0:
        return failed
    grid = ms.make_grid(v.min(axis=0), v.max(axis=0), kw.get('cell'), report['resolution'])
    assert grid[1] == report['cell'] and grid[2] == report['dims']
    origin, h, dims = grid
    cluster, cell_key = ms.host_clusters(v, grid)
    g, key = ms.host_face_keys(f, cluster)
    used = np.unique(g[key >= 0])                     # (the duplicate pass drops faces, never a cluster)
    if len(used) != len(out_v):
        failed.append('the clusters the faces name')
        return failed
    cells = np.stack([cell_key % dims[0], (cell_key // dims[0]) % dims[1], cell_key // (dims[0] * dims[1])], axis=1).astype(np.float64)[used]
    lo, hi = np.asarray(origin) + cells * h, np.asarray(origin) + (cells + 1.0) * h
    if not ((out_v >= lo) & (out_v <= hi)).all():
        failed.append('in its cell')
    at = np.full(len(cell_key), -1)
    at[used] = np.arange(len(used))
    member = at[cluster] >= 0
    dist = np.sqrt(((v[member] - out_v[at[cluster[member]]]) ** 2).sum(axis=1))
    diagonal = math.sqrt(sum((float(v[:, a].max()) - origin[a]) ** 2 for a in range(3)))
    if not (dist <= math.sqrt(3.0) * h + 1e-12 * diagonal).all():
        failed.append('within sqrt(3) h')
    return failed


@pytest.mark.parametrize('index', range(len(RUNS)), ids=[run_id(r) for r in RUNS])
def test_properties_of_the_definition(index):
    name, kw = RUNS[index]
    v, f = case(name)
    out_v, out_f, report = host_result(index)
    assert out_v.dtype == np.float64 and out_f.dtype == np.int64 and out_v.shape[1:] == (3,) and out_f.shape[1:] == (3,)
    assert failed_properties(v, f, out_v, out_f, report, kw) == []
    assert report['resolution'] == kw.get('resolution') and report['probes'] == []


def test_what_the_cases_are_there_for():
    by_id = {run_id(r): host_result(i)[2] for i, r in enumerate(RUNS)}
    assert case('cube16')[0].shape == (1538, 3) and case('cube16')[1].shape == (3072, 3)
    assert by_id['one_triangle-c4']['n_faces'] == 0 and by_id['one_triangle-c4']['n_vertices'] == 0 and by_id['one_triangle-c4']['n_clusters'] == 1
    assert by_id['one_triangle-r2']['n_faces'] == 1 and by_id['one_triangle-r2']['n_vertices'] == 3
    assert by_id['five_points-r2']['n_vertices'] == 0 and by_id['five_points-r2']['n_clusters'] > 0
    assert by_id['cube16-r2']['n_clusters'] == 26 and 3 * 3072 / 26 > 300                 # long corner runs
    assert by_id['cube16-r34']['n_faces'] == 3072 and by_id['cube16-r34']['n_vertices'] == 1538   # almost no merging: none
    assert all(by_id['cube16-r%d' % n]['n_clamped'] == 0 for n in (2, 4, 5, 34))
    assert sum(by_id['cube16_rotated-r%d' % n]['n_clamped'] > 0 for n in ROTATED_RESOLUTIONS) >= 3
    assert by_id['cube16_messy-r34']['n_faces_duplicate'] == 3 and by_id['cube16_messy-r34']['n_faces_degenerate'] == 1
    assert by_id['cube16_messy-r34']['n_clusters'] == by_id['cube16_messy-r34']['n_vertices'] + 4     # the unreferenced vertices
    slab = by_id['slab-c%g' % SLAB_H]
    assert slab['n_faces_duplicate'] == 256 and slab['n_faces'] == 256 and slab['n_faces_degenerate'] == 128
    out_f = host_result([run_id(r) for r in RUNS].index('slab-c%g' % SLAB_H))[1]
    triples = {tuple(t) for t in rotated_triples(out_f)}
    assert all((t[0], t[2], t[1]) in triples for t in triples)                             # every face has its opposite: both sides stay


def _corner_figures(n, **wrong):
    """(distance of the corner cluster's vertex from the cube's corner, distance of its centroid) / h for the eight corners."""
    v, f = case('cube16')
    grid = ms.make_grid(v.min(axis=0), v.max(axis=0), None, n)
    h = grid[1]
    cluster, cell_key = ms.host_clusters(v, grid)
    x, _ = ms.host_positions(v, f, cluster, cell_key, grid, **wrong)
    x0 = ms.host_quadrics(v, f, cluster, len(cell_key))[0]
    corners = np.nonzero((np.abs(v) == 1.0).all(axis=1))[0]
    assert len(corners) == 8 and len(set(cluster[corners])) == 8
    k = cluster[corners]
    alone = np.bincount(cluster)[k] == 1
    return np.sqrt(((x[k] - v[corners]) ** 2).sum(axis=1)) / h, np.sqrt(((x0[k] - v[corners]) ** 2).sum(axis=1)) / h, alone


@pytest.mark.parametrize('n', [4, 5])
def test_corner_gate(n):
    """Three equally weighted orthogonal planes leave a residual of 3 regularisation of the centroid's offset (1e-3 h here); the gate
    leaves a factor ten.  The centroid itself is a quarter of a cell and more away and fails the same gate.  The grid rule
    dims = floor(extent / h) + 1 puts the vertices AT the maximum into a layer of cells of their own (2 / h is exact here), so the
    corner (1, 1, 1) is alone in its cell: there the centroid is the corner itself and has nothing to show; the other seven
    clusters hold 5 to 25 vertices."""
    vertex, centroid, alone = _corner_figures(n)
    print('resolution %d: corner clusters %.2e .. %.2e h from the corner, their centroids %.3f .. %.3f h' % (
        n, vertex.min(), vertex.max(), centroid[~alone].min(), centroid[~alone].max()))
    assert (vertex < 0.01).all() and alone.sum() == 1 and (centroid[~alone] >= 0.25).all() and centroid[alone][0] == 0.0
    wrong, _, _ = _corner_figures(n, minimiser=False)
    assert (wrong[~alone] >= 0.25).all()              # the wrong formulation, the centroid in place of the minimiser, fails the gate


def test_flat_regions_stay_on_their_plane():
    v, f = case('cube16')
    for n in (4, 5):
        grid = ms.make_grid(v.min(axis=0), v.max(axis=0), None, n)
        cluster, cell_key = ms.host_clusters(v, grid)
        x, _ = ms.host_positions(v, f, cluster, cell_key, grid)
        on_side = np.abs(v) == 1.0
        interior = on_side.sum(axis=1) == 1
        checked = 0
        for k in range(len(cell_key)):
            members = np.nonzero(cluster == k)[0]
            if interior[members].all() and len(set(map(tuple, on_side[members]))) == 1:
                axis = int(on_side[members[0]].argmax())
                assert abs(x[k, axis] - v[members[0], axis]) <= 1e-12
                checked += 1
        assert checked >= 6


def test_wrong_formulations_fail_the_same_checks():
    v, f = case('slab')
    out = ms.host_simplify(v, f, cell=SLAB_H, deduplicate=False)
    assert 'a rotated triple twice' in failed_properties(v, f, *out, dict(cell=SLAB_H))
    v, f = case('cube16_rotated')
    seen = 0
    for n in ROTATED_RESOLUTIONS:
        right = host_result(RUNS.index(('cube16_rotated', dict(resolution=n))))
        if right[2]['n_clamped'] == 0:
            continue
        out = ms.host_simplify(v, f, resolution=n, clamp=False)
        # (a clamped cluster no face names does not show in the output)
        moved = out[0].tobytes() != right[0].tobytes()
        assert ('in its cell' in failed_properties(v, f, *out, dict(resolution=n))) == moved
        seen += moved
    assert seen >= 3


@pytest.mark.parametrize('target', [200, 2000, 10000])
def test_target_faces(target):
    v, f = case('sphere')
    out_v, out_f, report = ms.host_simplify(v, f, target_faces=target)
    assert 0 < report['n_faces'] == len(out_f) <= target and 'target_missed' not in report and 'unchanged' not in report
    assert failed_properties(v, f, out_v, out_f, report, {}) == []

    def count(n):           # the stated search, restated here on whole simplifications
        return ms.host_simplify(v, f, resolution=n)[2]['n_faces']
    probes = [(ms.MAX_RESOLUTION, count(ms.MAX_RESOLUTION)), (1, count(1))]
    assert probes[0][1] > target >= probes[1][1]
    lo, hi = 1, ms.MAX_RESOLUTION
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probes.append((mid, count(mid)))
        if probes[-1][1] <= target:
            lo = mid
        else:
            hi = mid
    assert report['probes'] == probes and report['resolution'] == lo
    again = ms.host_simplify(v, f, resolution=lo)
    assert again[0].tobytes() == out_v.tobytes() and np.array_equal(again[1], out_f)


def test_target_faces_unchanged_and_missed():
    v, f = case('sphere')
    for target in (len(f), len(f) + 5):
        out_v, out_f, report = ms.host_simplify(v, f, target_faces=target)
        assert report['unchanged'] is True and out_v.tobytes() == v.tobytes() and np.array_equal(out_f, f) and report['probes'] == []
    v, f = case('cube16')    # its sides x, y, z = 1 are cells of their own at resolution 1: 8 clusters, a closed surface of 12 faces
    out_v, out_f, report = ms.host_simplify(v, f, target_faces=1)
    assert report['target_missed'] is True and report['resolution'] == 1 and report['n_faces'] == len(out_f) == 12
    assert report['probes'] == [(ms.MAX_RESOLUTION, 3072), (1, 12)]
    mesh, report = ms.simplify_mesh((v, f), target_faces=len(f), device='cpu')
    assert report['unchanged'] and mesh.vertices.tobytes() == v.tobytes()


def test_argument_errors(monkeypatch):
    v, f = case('cube16')
    for kw in (dict(), dict(cell=0.5, resolution=4), dict(target_faces=10, cell=0.5), dict(cell=0.0), dict(cell=-1.0),
               dict(resolution=0), dict(resolution=ms.MAX_RESOLUTION + 1), dict(target_faces=0), dict(resolution=4, regularisation=0.0),
               dict(cell=1e-5)):
        with pytest.raises(ValueError):
            ms.host_simplify(v, f, **kw)
    bad = v.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        ms.host_simplify(bad, f, resolution=4)
    bad[7, 1] = np.inf
    with pytest.raises(ValueError, match='not finite'):
        ms.host_simplify(bad, f, resolution=4)
    for index in (-1, len(v)):
        wrong = f.copy()
        wrong[100, 2] = index
        with pytest.raises(ValueError, match='refers to vertex'):
            ms.host_simplify(v, wrong, resolution=4)
    monkeypatch.setattr(ms, 'MAX_CLUSTERS', 100)
    assert ms.host_simplify(v, f, resolution=4)[2]['n_clusters'] == 98
    with pytest.raises(ValueError, match='coarser cell'):
        ms.host_simplify(v, f, resolution=5)
    report = ms.host_simplify(v, f, target_faces=1000)[2]          # beyond the limit a probe counts as +inf
    assert report['probes'][0] == (ms.MAX_RESOLUTION, math.inf) and report['n_clusters'] <= 100 and report['n_faces'] <= 1000


def test_degenerate_sizes():
    v, f = case('empty')
    for kw in (dict(resolution=3), dict(cell=0.5), dict(target_faces=5)):
        out_v, out_f, report = ms.host_simplify(v, f, **kw)
        assert out_v.shape == (0, 3) and out_f.shape == (0, 3) and report['n_faces'] == 0 and report['n_vertices'] == 0
    v, f = case('five_points')
    out_v, out_f, report = ms.host_simplify(v, f, resolution=2)
    assert out_v.shape == (0, 3) and out_f.shape == (0, 3) and out_f.dtype == np.int64 and 1 <= report['n_clusters'] <= 5
    one = np.zeros((4, 3)) + 0.25                                   # zero extent on every axis: one cell with h = 1
    out_v, out_f, report = ms.host_simplify(one, np.array([[0, 1, 2], [1, 2, 3]]), resolution=7)
    assert report['cell'] == 1.0 and report['dims'] == (1, 1, 1) and report['n_clusters'] == 1 and report['n_faces_degenerate'] == 2
    mesh, report = ms.simplify_mesh(case('one_triangle'), resolution=2)
    # h = 0.5, dims (3, 3, 2): the corners (0, 0, 0), (1, 0, 0), (0, 1, 0.5) have the keys 0, 2, 15, so the clusters keep the vertex order
    # and the face its corner order; its plane is all the quadric knows, and every corner already lies on it
    assert report['dims'] == (3, 3, 2) and mesh.faces.tolist() == [[0, 1, 2]]
    assert np.abs(mesh.vertices - case('one_triangle')[0]).max() < 1e-12
