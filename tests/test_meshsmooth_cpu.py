"""The numpy definition of the smoothing (psnerf_amd/meshsmooth.py:host_smooth) against known answers: exact cases on integer
lattices, the bits of held vertices, the orderings between the plain Laplacian and the lambda | mu filter measured on a
marching-cubes mesh, the extractor's new arguments on the host path and the command-line tool.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

from tests.helpers import ROOT
from tests import mesh_fields as mf
from tests import meshtopo_cases as tc
from psnerf_amd import meshsmooth as ms, meshtopo as mt
from psnerf_amd.meshcore import Mesh


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(ROOT, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_arguments_are_checked():
    v, f = tc.case('tet')
    for kw in (dict(lam=0.0), dict(lam=1.5), dict(lam=float('nan')), dict(mu=-0.5), dict(mu=-0.4), dict(mu=0.6), dict(mu=float('nan')),
               dict(iterations=-1), dict(iterations=1.5), dict(pin='rim'), dict(pin=np.zeros(3, dtype=bool)), dict(pin=np.zeros(4))):
        with pytest.raises(ValueError, match='smooth'):
            ms.host_smooth(v, f, **kw)
        with pytest.raises(ValueError, match='smooth'):
            ms.smooth_mesh((v, f), **kw)
    with pytest.raises(ValueError, match='a face refers to vertex'):
        ms.host_smooth(*tc.OUT_OF_RANGE)
    with pytest.raises(ValueError, match='weight'):
        ms.smooth_mesh((v, f), normals='angle')
    x, report = ms.host_smooth(v, f, iterations=0)
    assert x.tobytes() == v.tobytes() and report['iterations'] == 0 and report['max_displacement'] == 0.0
    ms.host_smooth(v, f, lam=1.0, mu=-1.0000001)                   # the ends of the admissible ranges


@pytest.mark.parametrize('lam,mu', [(0.5, -0.53), (1.0, -1.25), (0.3, None), (0.7071, -0.9)])
def test_planar_lattice_patch_does_not_move(lam, mu):
    """Every interior vertex of the patch has six neighbours that sum to six times the vertex, exactly, in integers: the mean is the
    vertex, the difference +0.0 and the vertex keeps its bits under any lam, mu; the rim is pinned."""
    v, f = tc.case('patch')
    shifted = v * np.array([3.0, 5.0, 0.0]) + np.array([-7.0, 11.0, 2.0])                 # (still integers; not symmetric)
    x, report = ms.host_smooth(shifted, f, iterations=4, lam=lam, mu=mu)
    assert x.tobytes() == shifted.tobytes()
    assert report['n_pinned'] == 2 * (6 + 4) and report['n_isolated'] == 0 and report['max_displacement'] == 0.0
    assert report['area_before'] == report['area_after'] == 24.0 * 15.0
    lifted = shifted.copy()
    centre = 3 * 5 + 2                                                                    # vertex (3, 2): interior
    lifted[centre, 2] += 6.0
    y, _ = ms.host_smooth(lifted, f, iterations=1, lam=0.5, mu=None)
    assert y[centre].tolist() == [shifted[centre, 0], shifted[centre, 1], 5.0]            # 8 + 0.5 (2 - 8)
    ring_start, ring = mt.host_rings(mt.host_edges(f, len(v))['edges'], len(v))
    mine = ring[ring_start[centre]:ring_start[centre + 1]]
    assert len(mine) == 6 and all(y[w, 2] == 2.5 for w in mine)                           # all interior: 2 + 0.5 ((8 + 5 * 2) / 6 - 2)


def test_a_ring_of_four_lands_on_the_exact_value():
    v = np.array([[1, 2, 3], [4, 0, -2], [0, 4, 2], [2, -2, -6], [2, 2, 2]], dtype=np.float64)       # the ring sums to (8, 4, -4)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], dtype=np.int64)
    x, report = ms.host_smooth(v, f, iterations=1, lam=0.5, mu=None, pin=None)
    assert x[0].tolist() == [1.5, 1.5, 1.0]                                                # x + 0.5 ((2, 1, -1) - x)
    assert x[1].tolist() == [4 + 0.5 * ((1 + 0 + 2) / 3 - 4), 0 + 0.5 * ((2 + 4 + 2) / 3 - 0), -2 + 0.5 * ((3 + 2 + 2) / 3 + 2)]
    assert report['n_pinned'] == 0
    held, report = ms.host_smooth(v, f, iterations=3, pin='boundary')                      # the four rim vertices hold, the centre moves
    assert held[1:].tobytes() == v[1:].tobytes() and report['n_pinned'] == 4
    pair, _ = ms.host_smooth(v, f, iterations=1, lam=0.5, mu=-1.0, pin='boundary')
    assert pair[0].tolist() == [1.0, 2.0, 3.0]                                             # x1 = (1.5, 1.5, 1), then x1 - ((2, 1, -1) - x1)


def test_pinned_and_isolated_vertices_keep_their_bits():
    v, f = tc.case('oddities')
    v = v.copy()
    v[3] = [-0.0, 5e-324, -2.5e-310]                                                      # a vertex of the torus: pinned below
    mask = np.zeros(len(v), dtype=bool)
    mask[[3, 7]] = True
    x, report = ms.host_smooth(v, f, iterations=3, pin=mask)
    isolated = np.diff(mt.host_rings(mt.host_edges(f, len(v))['edges'], len(v))[0]) == 0
    assert isolated.sum() == 2 and report['n_isolated'] == 2 and report['n_pinned'] == 2
    held = mask | isolated
    assert x[held].tobytes() == v[held].tobytes() and np.signbit(x[3, 0]) and x[3, 1] == 5e-324
    assert (x[~held] != v[~held]).any(axis=1).all()
    free, _ = ms.host_smooth(v, f, iterations=1, pin=None)
    assert free[isolated].tobytes() == v[isolated].tobytes() and (free[3] != v[3]).any()


def test_taubin_keeps_the_volume_the_laplacian_shrinks():
    """The four relations measured on sphere_rod_torus (11 410 vertices): orderings, not thresholds."""
    v, f = tc.case('sphere_rod_torus')
    table = tc.host('sphere_rod_torus')[0]
    ring_start, ring = tc.host('sphere_rod_torus')[1]
    v0 = tc.host('sphere_rod_torus')[3]['volume']
    lap = {}
    for n in (1, 5, 10):
        x, report = ms.host_smooth(v, f, iterations=2 * n, lam=0.5, mu=None)
        lap[n] = (x, report['volume_after'])
        assert report['volume_before'] == v0 and report['n_pinned'] == 0
    taubin, report = ms.host_smooth(v, f, iterations=10)
    u0, u_lap, u_taubin = ms.host_umbrella(v, ring_start, ring), ms.host_umbrella(lap[10][0], ring_start, ring), ms.host_umbrella(taubin, ring_start, ring)
    print('volume / input: Laplacian %.4f %.4f %.4f after 2, 10, 20 steps; Taubin %.4f after 10 pairs; umbrella %.4f -> %.4f (Laplacian), %.4f (Taubin)'
          % (lap[1][1] / v0, lap[5][1] / v0, lap[10][1] / v0, report['volume_after'] / v0, u0, u_lap, u_taubin))
    assert v0 > lap[1][1] > lap[5][1] > lap[10][1] > 0.0
    assert (lap[10][0].min(axis=0) >= v.min(axis=0)).all() and (lap[10][0].max(axis=0) <= v.max(axis=0)).all()
    assert abs(1.0 - report['volume_after'] / v0) < abs(1.0 - lap[10][1] / v0)
    assert u_lap < u0 and u_taubin < u0
    assert mt.host_report(taubin, f, table)['is_oriented']


def test_smooth_mesh_on_the_host_path():
    v, f = tc.case('torus')
    x, report = ms.host_smooth(v, f, iterations=3)
    mesh, same = ms.smooth_mesh(Mesh(v, f, vertex_normals=np.ones_like(v)), iterations=3)
    assert mesh.vertices.tobytes() == x.tobytes() and np.array_equal(mesh.faces, f) and mesh.vertex_normals is None and same == report
    with_normals, _ = ms.smooth_mesh((v, f), iterations=3, normals='uniform')
    assert with_normals.vertex_normals.tobytes() == mt.host_vertex_normals(x, f, 'uniform').tobytes()
    assert sorted(report) == ['area_after', 'area_before', 'iterations', 'max_displacement', 'mean_displacement', 'n_isolated', 'n_pinned',
                              'volume_after', 'volume_before']
    assert 0.0 < report['mean_displacement'] <= report['max_displacement']


def test_extractor_on_the_host_path():
    from psnerf_amd.stage1.extracting import Extractor3D
    kw = dict(device='cpu', resolution0=16, upsampling_steps=1, points_batch_size=3000)
    plain, pstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(32)), **kw).generate_mesh()
    same, sstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(32)), smooth_iterations=None, smooth_lambda=0.9, smooth_mu=-2.0, **kw).generate_mesh()
    assert same.vertices.tobytes() == plain.vertices.tobytes() and same.faces.tobytes() == plain.faces.tobytes()
    assert sorted(pstats) == sorted(sstats) and 'smooth_iterations' not in sstats
    smooth, stats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(32)), smooth_iterations=2, **kw).generate_mesh()
    want, report = ms.host_smooth(plain.vertices, plain.faces, 2)
    assert smooth.faces.tobytes() == plain.faces.tobytes() and smooth.vertices.tobytes() == want.tobytes() != plain.vertices.tobytes()
    assert stats['smooth_iterations'] == 2 and stats['n_vertices_pinned'] == 0 and stats['time (smooth)'] >= 0.0
    assert stats['smooth_max_displacement'] == report['max_displacement'] > 0.0
    topology = mt.mesh_report(smooth)
    assert topology['is_watertight'] and topology['is_oriented'] and topology == dict(mt.mesh_report(plain), area=topology['area'], volume=topology['volume'])


def test_extract_mesh_tool_smooths_on_the_host_path(tmp_path, capsys):
    """tools/extract_mesh.py --no-cuda --smooth 2 writes host_smooth of what it writes without the option."""
    import torch
    import yaml
    from oracle.stage1 import NeuralNetwork
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.meshcore import load_mesh
    from psnerf_amd.synthetic import stage1_cfg
    cfg = stage1_cfg('bear')
    cfg['extraction'] = {'resolution': 16, 'upsampling_steps': 0, 'refinement_step': 0}
    exp = tmp_path / 'out' / 'bear' / 'test_1'
    os.makedirs(str(exp / 'models'))
    with open(str(exp / 'config.yaml'), 'w') as fh:
        yaml.safe_dump(cfg, fh)
    torch.manual_seed(0)
    CheckpointIO(str(exp / 'models'), model=NeuralNetwork(cfg)).save('model.pt')
    args = ['--obj_name', 'bear', '--exp_folder', str(tmp_path / 'out'), '--mesh_extension', 'obj', '--no-cuda']
    plain = load_mesh(_tool('extract_mesh').main(args + ['--test_out_dir', str(tmp_path / 'a')]))
    assert 'smoothed' not in capsys.readouterr().out
    smooth = load_mesh(_tool('extract_mesh').main(args + ['--test_out_dir', str(tmp_path / 'b'), '--smooth', '2']))
    assert 'smoothed by 2 lambda | mu pairs: 0 vertices pinned' in capsys.readouterr().out
    assert len(plain.faces) > 100 and np.array_equal(smooth.faces, plain.faces)
    assert smooth.vertices.tobytes() == ms.host_smooth(plain.vertices, plain.faces, 2)[0].tobytes() != plain.vertices.tobytes()


def test_the_tool_on_a_small_obj(tmp_path, capsys):
    v, f = tc.case('torus')
    src, dst = str(tmp_path / 'in.obj'), str(tmp_path / 'out.obj')
    Mesh(v, f).export(src)
    from psnerf_amd.meshcore import load_mesh
    _, report = _tool('smooth_mesh').main([src, dst, '--smooth', '3', '--report', '--normals', 'area'])
    out = capsys.readouterr().out
    got = load_mesh(dst)
    want, want_report = ms.host_smooth(load_mesh(src).vertices, f, 3)
    assert got.vertices.tobytes() == want.tobytes() and np.array_equal(got.faces, f) and got.vertex_normals is not None and report == want_report
    assert 'before: watertight and oriented' in out and 'after:  watertight and oriented' in out and '3 lambda | mu pairs, 0 vertices pinned' in out
    _tool('smooth_mesh').main([src, dst, '--smooth', '2', '--laplacian', '--no-pin', '--smooth-lambda', '0.25'])
    assert '2 Laplacian steps' in capsys.readouterr().out
    assert load_mesh(dst).vertices.tobytes() == ms.host_smooth(load_mesh(src).vertices, f, 2, 0.25, None, None)[0].tobytes()
