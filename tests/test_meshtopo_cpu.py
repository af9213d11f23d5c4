"""The numpy definition of the mesh connectivity (psnerf_amd/meshtopo.py:host_*) against known answers: constructed meshes whose edge
classes follow from how they were built, three marching-cubes meshes with the values computed on the CPU, an independent
formulation of the edge table (a dictionary of edges), meshocclude.area_weighted_normals byte for byte, and the report through
evaluate_mesh and its tool.  No GPU."""
import collections
import importlib.util
import os

import numpy as np
import pytest

from tests.helpers import ROOT
from tests import mesh_fields as mf
from tests import meshtopo_cases as tc
from psnerf_amd import meshtopo as mt
from psnerf_amd.meshocclude import area_weighted_normals


def _by_dictionary(f, n_v):
    """The edge table by a dictionary over the half-edges in ascending h: an independent formulation."""
    runs = collections.OrderedDict()
    degenerate = 0
    for t, (i, j, k) in enumerate(f.tolist()):
        if i == j or j == k or i == k:
            degenerate += 1
            continue
        for c, (a, b) in enumerate(((i, j), (j, k), (k, i))):
            runs.setdefault((min(a, b), max(a, b)), []).append((3 * t + c, a < b))
    keys = sorted(runs)
    halfedge_edge = np.full(3 * len(f), -1, dtype=np.int64)
    for e, key in enumerate(keys):
        for h, _ in runs[key]:
            halfedge_edge[h] = e
    count = np.array([len(runs[k]) for k in keys], dtype=np.int32)
    forward = np.array([sum(fw for _, fw in runs[k]) for k in keys], dtype=np.int32)
    return np.array(keys, dtype=np.int64).reshape(-1, 2), count, forward, halfedge_edge, degenerate


@pytest.mark.parametrize('name', tc.NAMES)
def test_edge_table_against_a_dictionary_of_edges(name):
    v, f = tc.case(name)
    table = tc.host(name)[0]
    edges, count, forward, halfedge_edge, degenerate = _by_dictionary(f, len(v))
    assert table['edges'].dtype == np.int64 and table['edges'].shape == edges.shape and np.array_equal(table['edges'], edges)
    assert table['count'].dtype == np.int32 and np.array_equal(table['count'], count)
    assert table['forward'].dtype == np.int32 and np.array_equal(table['forward'], forward)
    assert table['halfedge_edge'].dtype == np.int64 and np.array_equal(table['halfedge_edge'], halfedge_edge)
    assert table['counters'].tolist() == [int((count == 1).sum()), int((count > 2).sum()), int(((count == 2) & (forward != 1)).sum()), degenerate]
    assert (np.diff(edges[:, 0] * max(len(v), 1) + edges[:, 1]) > 0).all() and (edges[:, 0] < edges[:, 1]).all()


@pytest.mark.parametrize('name', sorted(tc.KNOWN))
def test_report_of_the_constructed_meshes(name):
    v, f = tc.case(name)
    report = tc.host(name)[3]
    for key, want in tc.KNOWN[name].items():
        assert report[key] == want and type(report[key]) is type(want), '%s: %s = %r, expected %r' % (name, key, report[key], want)
    assert report['n_vertices'] == len(v) and report['n_faces'] == len(f)
    assert report['euler'] == (len(v) - report['n_vertices_unreferenced']) - report['n_edges'] + (len(f) - report['n_faces_degenerate'])
    assert report['is_oriented'] == (mf.is_closed_oriented(f) and len(f) > 0) or report['n_faces_degenerate'] > 0
    assert all(type(report[k]) is float for k in ('area', 'volume'))


def test_known_measures():
    tet = tc.host('tet')[3]
    assert abs(tet['volume'] - 1.0 / 6.0) < 1e-15 and abs(tet['area'] - (1.5 + 0.5 * np.sqrt(3.0))) < 1e-15
    flat = tc.host('patch')[3]
    assert flat['area'] == 24.0 and flat['volume'] == 0.0
    for name in ('sphere_rod_torus', 'checker16'):
        v, f = tc.case(name)
        area, volume = mf.area_volume(v, f)
        got = tc.host(name)[3]
        assert abs(got['area'] - area) <= 1e-12 * area and abs(got['volume'] - volume) <= 1e-12 * abs(volume) and got['volume'] > 0.0


@pytest.mark.parametrize('name', sorted(tc.MEASURED))
def test_report_of_the_marching_cubes_meshes(name):
    v, f = tc.case(name)
    report = tc.host(name)[3]
    assert tuple(report[k] for k in tc.MEASURED_KEYS) == tc.MEASURED[name]
    assert report['is_oriented'] == mf.is_closed_oriented(f)
    assert report['is_oriented'] == (name != 'ribbon') and report['is_watertight'] == (name != 'ribbon')


@pytest.mark.parametrize('name', tc.NAMES)
def test_rings_and_corner_runs(name):
    v, f = tc.case(name)
    table, (ring_start, ring), (corner_start, corner), _ = tc.host(name)
    n_v, n_f = len(v), len(f)
    assert ring_start.dtype == ring.dtype == np.int64 and ring_start.shape == (n_v + 1,) and ring.shape == (2 * len(table['edges']),)
    assert ring_start[0] == 0 and ring_start[-1] == len(ring) and (np.diff(ring_start) >= 0).all()
    live = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    for u in range(n_v) if n_v <= 400 else np.random.RandomState(0).randint(0, n_v, 200):
        mine = ring[ring_start[u]:ring_start[u + 1]]
        assert (np.diff(mine) > 0).all()                                              # unique and ascending
        assert set(mine.tolist()) == set(live[(live == u).any(axis=1)].reshape(-1).tolist()) - {u}
    assert corner_start.shape == (n_v + 1,) and corner.shape == (3 * n_f,) and sorted(corner.tolist()) == list(range(3 * n_f))
    owner = f.T.reshape(-1)[corner] if n_f else np.zeros(0, dtype=np.int64)
    assert np.array_equal(owner, np.repeat(np.arange(n_v), np.diff(corner_start)))
    same = owner[1:] == owner[:-1]
    assert (np.diff(corner)[same] > 0).all()                                          # within a run ascending j = k F + f: ascending (k, f)


@pytest.mark.parametrize('name', tc.NAMES)
def test_area_normals_are_area_weighted_normals_bytewise(name):
    v, f = tc.case(name)
    got = mt.host_vertex_normals(v, f, 'area')
    assert got.dtype == np.float64 and got.tobytes() == area_weighted_normals(v, f).tobytes()
    uniform = mt.host_vertex_normals(v, f, 'uniform')
    length = np.sqrt((uniform * uniform).sum(axis=1))
    assert np.isfinite(uniform).all() and (np.abs(length[length > 0] - 1.0) < 1e-12).all()
    assert np.array_equal(length > 0, np.sqrt((got * got).sum(axis=1)) > 0) or name == 'oddities'
    with pytest.raises(ValueError, match='weight'):
        mt.host_vertex_normals(v, f, 'angle')


def test_uniform_normals_known_answer():
    """A vertex shared by a large and a small face at right angles: 'area' leans to the large face, 'uniform' sits in the middle."""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float64)
    f = np.array([[0, 1, 2], [0, 3, 4]], dtype=np.int64)           # normals (0, 0, 16) and (1, 0, 0)
    area, uniform = mt.host_vertex_normals(v, f, 'area'), mt.host_vertex_normals(v, f, 'uniform')
    assert np.array_equal(area[0], np.array([1.0, 0.0, 16.0]) / np.sqrt(257.0))
    assert np.array_equal(uniform[0], np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0))
    assert np.array_equal(uniform[1], [0.0, 0.0, 1.0]) and np.array_equal(uniform[3], [1.0, 0.0, 0.0])


def test_out_of_range_indices_raise():
    v, f = tc.OUT_OF_RANGE
    for call in (lambda: mt.host_edges(f, len(v)), lambda: mt.host_report(v, f), lambda: mt.host_corner_runs(f, len(v)),
                 lambda: mt.host_vertex_normals(v, f), lambda: mt.mesh_report((v, f)), lambda: mt.edges((v, f)), lambda: mt.rings((v, f)),
                 lambda: mt.vertex_normals((v, f))):
        with pytest.raises(ValueError, match='a face refers to vertex'):
            call()


def test_public_functions_take_the_host_path_for_cpu_inputs():
    import torch
    v, f = tc.case('torus')
    table, ring, corner, report = tc.host('torus')
    for mesh in ((v, f), (torch.from_numpy(v.copy()), torch.from_numpy(f.copy()))):
        got = mt.edges(mesh)
        assert all(np.array_equal(got[k], table[k]) for k in table)
        assert mt.mesh_report(mesh) == report
        assert all(np.array_equal(a, b) for a, b in zip(mt.rings(mesh), ring))
        assert all(np.array_equal(a, b) for a, b in zip(mt.corner_runs(mesh), corner))
        assert mt.vertex_normals(mesh).tobytes() == area_weighted_normals(v, f).tobytes()


def test_evaluate_mesh_report_and_its_tool(tmp_path, capsys):
    from psnerf_amd.meshcore import Mesh
    from psnerf_amd.mesheval import evaluate_mesh
    v, f = tc.case('torus')
    hole = f[1:]
    kw = dict(num_samples=500, iou_points=300)
    plain = evaluate_mesh(Mesh(v, hole), Mesh(v, f), rng=np.random.RandomState(0), **kw)
    with_report = evaluate_mesh(Mesh(v, hole), Mesh(v, f), rng=np.random.RandomState(0), report=True, **kw)
    assert 'pred_topology' not in plain and sorted(set(with_report) - set(plain)) == ['gt_topology', 'pred_topology']
    assert all(repr(plain[k]) == repr(with_report[k]) for k in plain if k != 'raw')
    assert all(np.array_equal(np.asarray(plain['raw'][k]), np.asarray(with_report['raw'][k])) for k in plain['raw'])
    assert with_report['gt_topology'] == tc.host('torus')[3] and with_report['gt_topology']['is_oriented']
    assert with_report['pred_topology']['n_boundary_edges'] == 3 and not with_report['pred_topology']['is_watertight']
    a, b = str(tmp_path / 'pred.obj'), str(tmp_path / 'gt.obj')
    Mesh(v, hole).export(a)
    Mesh(v, f).export(b)
    spec = importlib.util.spec_from_file_location('evaluate_mesh_tool', os.path.join(ROOT, 'tools', 'evaluate_mesh.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main([a, b, '--samples', '500', '--iou-points', '300', '--seed', '0', '--topology', '--device', 'cpu'])
    out = capsys.readouterr().out
    assert 'pred topology' in out and '3 boundary' in out and 'gt   topology      watertight and oriented:' in out
    assert 'pred topology      NOT watertight:' in out
