"""Mesh clean-up without a GPU (psnerf_amd/meshclean.py): the numpy definition of connected components against an independent
union-find, the per-component table, the selection rules, cleaning, the extractor's new arguments on the host path, the two
command-line tools' new flags, and the argument validation of the new C entries."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import ROOT
from tests import mesh_fields as mf
from tests.meshclean_cases import CASES, case, ribbon
from psnerf_amd import meshclean as mc
from psnerf_amd.stage1.extracting import Extractor3D, Mesh


def union_find_labels(faces, n_vertices):
    """Independent of the module: a sequential union-find (union by smaller index, path compression), pure Python."""
    parent = list(range(n_vertices))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    for tri in np.asarray(faces).tolist():
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2])):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n_vertices)], dtype=np.int64)


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_components_against_an_independent_union_find(name):
    v, f = case(name)
    labels = mc.host_components(f, len(v))
    assert labels.dtype == np.int64 and labels.shape == (len(v),)
    assert np.array_equal(labels, union_find_labels(f, len(v)))
    want = CASES[name]
    assert len(f) == want['faces'] and len(v) == want['vertices'] and len(np.unique(labels)) == want['classes']
    # an unreferenced vertex keeps its own index
    unreferenced = np.setdiff1d(np.arange(len(v)), f.reshape(-1))
    assert np.array_equal(labels[unreferenced], unreferenced)


@pytest.mark.parametrize('name', sorted(CASES))
def test_component_table_counts_and_areas(name):
    v, f = case(name)
    labels = mc.host_components(f, len(v))
    t = mc.host_component_table(v, f, labels)
    assert all(t[k].dtype == np.int64 for k in ('label', 'n_vertices', 'n_faces')) and t['area'].dtype == np.float64
    assert np.array_equal(t['label'], np.unique(labels[f[:, 0]])) and int(t['n_faces'].sum()) == len(f)
    assert int(t['n_vertices'].sum()) == int(np.isin(labels, t['label']).sum())
    for row, l in enumerate(t['label']):
        assert t['n_vertices'][row] == (labels == l).sum() and t['n_faces'][row] == (labels[f[:, 0]] == l).sum()
    area, _ = mf.area_volume(v, f)
    assert abs(t['area'].sum() - area) <= max(len(f), 1) * 2.0 ** -50 * area
    if 'largest' in CASES[name]:
        assert sorted(t['n_faces'].tolist(), reverse=True)[:len(CASES[name]['largest'])] == CASES[name]['largest']


def test_the_ribbon_needs_few_rounds():
    """Hook-and-jump does not grow with the diameter: 9 rounds where neighbour-to-neighbour propagation needs 1734."""
    v, f = ribbon()
    _, rounds = mc.host_components(f, len(v), return_rounds=True)
    assert rounds <= 16


def _table(n_faces, area=None, label=None):
    n = len(n_faces)
    return {'label': np.asarray(label if label is not None else np.arange(n) * 3, dtype=np.int64), 'n_vertices': np.ones(n, dtype=np.int64),
            'n_faces': np.asarray(n_faces, dtype=np.int64), 'area': np.asarray(area if area is not None else n_faces, dtype=np.float64)}


def test_select_rules():
    t = _table([5, 16, 100, 16, 2], area=[9.0, 1.0, 3.0, 2.0, 50.0])       # labels 0, 3, 6, 9, 12
    assert mc.select(t).tolist() == [0, 3, 6, 9, 12]
    assert mc.select(t, min_faces=5).tolist() == [0, 3, 6, 9] and mc.select(t, min_faces=17).tolist() == [6]
    assert mc.select(t, keep=1).tolist() == [6]
    assert mc.select(t, keep=2).tolist() == [3, 6]                          # 16 faces twice: the smaller label
    assert mc.select(t, keep=3).tolist() == [3, 6, 9] and mc.select(t, keep=99).tolist() == [0, 3, 6, 9, 12]
    assert mc.select(t, keep=1, by='area').tolist() == [12] and mc.select(t, keep=2, by='area').tolist() == [0, 12]
    assert mc.select(t, keep=1, by='area', min_faces=3).tolist() == [0]     # min_faces first, then the largest
    assert mc.select(t, keep=2, min_faces=101).tolist() == []
    tie = _table([4, 4, 4], area=[2.0, 2.0, 2.0], label=[7, 2, 5])
    assert mc.select(tie, keep=1).tolist() == [2] and mc.select(tie, keep=2, by='area').tolist() == [2, 5]
    with pytest.raises(ValueError):
        mc.select(t, keep=0)
    with pytest.raises(ValueError):
        mc.select(t, by='volume')


@pytest.mark.parametrize('name,kw', [('sphere_rod_torus', dict(keep=1)), ('checker16', dict(keep=2)), ('checker16_shuffled', dict(keep=3)),
                                     ('checker32', dict(min_faces=16)), ('sphere_rod_torus', dict(keep=1, by='area')), ('ribbon', dict(keep=1))])
def test_host_clean(name, kw):
    v, f = case(name)
    normals = np.random.RandomState(3).randn(len(v), 3).astype(np.float32)
    cv, cf, cn, report = mc.host_clean(v, f, normals, **kw)
    labels = mc.host_components(f, len(v))
    kept = mc.select(report['table'], **kw)
    face_keep = np.isin(labels[f[:, 0]], kept)
    used = np.unique(f[face_keep])
    assert cv.dtype == np.float64 and cf.dtype == np.int64 and cn.dtype == np.float32
    assert cv.tobytes() == v[used].tobytes() and cn.tobytes() == normals[used].tobytes()        # original order, bits untouched
    assert np.array_equal(used[cf], f[face_keep])                                               # re-indexed, order preserved
    assert report['n_components'] == len(report['table']['label']) and report['n_kept'] == len(kept)
    assert report['n_faces_removed'] == len(f) - len(cf) and report['n_vertices_removed'] == len(v) - len(cv)
    assert len(np.unique(mc.host_components(cf, len(cv)))) == len(kept)
    if name != 'ribbon':
        assert mf.is_closed_oriented(cf) and len(cf) < len(f)


def test_host_clean_known_answers():
    v, f = case('sphere_rod_torus')
    _, cf, _, report = mc.host_clean(v, f, keep=1)
    assert len(cf) == 14656 and report['n_faces_removed'] == 8160 and report['n_components'] == 2 and report['n_kept'] == 1
    _, ca, _, _ = mc.host_clean(v, f, keep=1, by='area')
    t = report['table']
    assert len(ca) == int(t['n_faces'][np.argmax(t['area'])])
    _, call, cn, rall = mc.host_clean(v, f)                                 # keep=None, min_faces=0: every face stays
    assert np.array_equal(call, f) and cn is None and rall['n_faces_removed'] == 0
    v16, f16 = case('checker16')
    _, c2, _, r2 = mc.host_clean(v16, f16, keep=2)
    t16 = r2['table']
    tied = t16['label'][t16['n_faces'] == 16]
    assert len(tied) == 2 and len(c2) == 16212 + 16 and mc.select(t16, keep=2).tolist() == sorted([int(t16['label'][np.argmax(t16['n_faces'])]), int(tied.min())])
    # the empty mesh and a mesh without faces
    ev, ef, _, er = mc.host_clean(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), keep=1)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and er['n_components'] == 0
    ev, ef, _, er = mc.host_clean(np.zeros((5, 3)), np.zeros((0, 3), dtype=np.int64), keep=1)
    assert ev.shape == (0, 3) and er['n_vertices_removed'] == 5


def test_out_of_range_index_raises():
    v = np.zeros((3, 3))
    for bad in ([[0, 1, 3]], [[0, -1, 2]]):
        with pytest.raises(ValueError):
            mc.host_components(np.array(bad), 3)
        with pytest.raises(ValueError):
            mc.host_clean(v, np.array(bad), keep=1)
        with pytest.raises(ValueError):
            mc.components(v, np.array(bad))


def test_public_functions_on_the_host_path():
    v, f = case('sphere_rod_torus')
    labels, table = mc.components(v, f)
    assert np.array_equal(labels, mc.host_components(f, len(v))) and table['n_faces'].tolist() == [14656, 8160]
    normals = np.random.RandomState(1).randn(len(v), 3)
    mesh, report = mc.clean_mesh(Mesh(v, f, vertex_normals=normals))
    hv, hf, hn, _ = mc.host_clean(v, f, normals, keep=1)
    assert isinstance(mesh, Mesh) and np.array_equal(mesh.vertices, hv) and np.array_equal(mesh.faces, hf)
    assert np.array_equal(mesh.vertex_normals, hn) and report['n_faces_removed'] == 8160
    mesh2, _ = mc.clean_mesh((torch.from_numpy(v.copy()), torch.from_numpy(f.copy())), keep=None, min_faces=10000)
    assert np.array_equal(mesh2.faces, hf) and mesh2.vertex_normals is None


def test_extractor_arguments_on_the_host_path():
    kw = dict(resolution0=16, upsampling_steps=2)
    plain, pstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), **kw).generate_mesh()
    same, sstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), keep_components=None, min_component_faces=0, **kw).generate_mesh()
    assert same.vertices.tobytes() == plain.vertices.tobytes() and np.array_equal(same.faces, plain.faces)
    assert 'n_components' not in sstats and sorted(sstats) == sorted(pstats)
    kept, stats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), keep_components=1, **kw).generate_mesh()
    hv, hf, _, report = mc.host_clean(plain.vertices, plain.faces, keep=1)
    assert kept.vertices.tobytes() == hv.tobytes() and np.array_equal(kept.faces, hf) and len(hf) < len(plain.faces)
    assert stats['n_components'] == report['n_components'] == 2 and stats['n_faces_removed'] == report['n_faces_removed']
    assert stats['time (components)'] >= 0.0 and mf.is_closed_oriented(kept.faces)
    small, _ = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), min_component_faces=10 ** 6, **kw).generate_mesh()
    assert small.is_empty and small.faces.shape == (0, 3)


def test_chamfer_tool_keep_components(tmp_path):
    from tests.test_chamfer_cpu import icosphere
    gt = icosphere(1.0, 2)
    far = icosphere(0.2, 1)
    pred = Mesh(np.concatenate([icosphere(1.0, 2).vertices, far.vertices + 5.0]), np.concatenate([gt.faces, far.faces + len(gt.vertices)]))
    a, b = gt.export(str(tmp_path / 'gt.ply')), pred.export(str(tmp_path / 'pred.obj'))
    tool = [sys.executable, os.path.join(ROOT, 'tools', 'chamfer_dist.py'), '--mesh_gt', a, '--mesh_pred', b, '--num_samples', '2000', '--seed', '0',
            '--no-cuda']
    value = lambda out: float([l for l in out.splitlines() if l.startswith('Chamfer')][0].split()[-1])
    with_floater = subprocess.check_output(tool).decode()
    cleaned = subprocess.check_output(tool + ['--keep-components', '1']).decode()
    assert 'components' not in with_floater and re.search(r'1 of 2 connected components kept, 80 faces removed', cleaned), cleaned
    assert value(with_floater) > 50.0 and value(cleaned) < 5.0      # the floater's samples are some 7 units away; without it: sampling noise


def test_extract_mesh_tool_flags(tmp_path, capsys):
    import yaml
    from oracle.stage1 import NeuralNetwork
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.synthetic import stage1_cfg
    spec = importlib.util.spec_from_file_location('extract_mesh_tool', os.path.join(ROOT, 'tools', 'extract_mesh.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cfg = stage1_cfg('bear')
    cfg['extraction'] = {'resolution': 8, 'upsampling_steps': 1, 'refinement_step': 0}
    exp = tmp_path / 'out' / 'bear' / 'test_1'
    os.makedirs(str(exp / 'models'))
    with open(str(exp / 'config.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f)
    torch.manual_seed(0)
    CheckpointIO(str(exp / 'models'), model=NeuralNetwork(cfg)).save('model.pt')
    args = ['--no-cuda', '--obj_name', 'bear', '--exp_folder', str(tmp_path / 'out'), '--mesh_extension', 'obj']
    from psnerf_amd.meshdist import load_mesh
    plain = load_mesh(tool.main(args + ['--test_out_dir', str(tmp_path / 'a')]))
    assert 'connected components' not in capsys.readouterr().out
    kept = load_mesh(tool.main(args + ['--test_out_dir', str(tmp_path / 'b'), '--keep-components', '1', '--min-component-faces', '4']))
    assert '1 connected components, 0 faces removed' in capsys.readouterr().out     # the sphere of the geometric initialisation
    assert np.array_equal(kept.vertices, plain.vertices) and np.array_equal(kept.faces, plain.faces)
    none = load_mesh(tool.main(args + ['--test_out_dir', str(tmp_path / 'c'), '--min-component-faces', '1000000']))
    assert len(none.faces) == 0


def test_argument_validation_of_the_clean_up_entries_needs_no_gpu():
    from psnerf_amd import hip
    lib = hip._lib
    dummy = ctypes.c_void_p(64)
    assert hip.CC_MAX_VERTICES == 2 ** 31 - 2 and hip.CC_E_INDEX == 1 and hip.CC_E_BOUND == 2
    rc = lib.psn_cc_label(dummy, 4, -1, dummy, dummy, dummy, None)
    assert rc == -1 and b'n_vertices' in lib.psn_last_error()
    rc = lib.psn_cc_label(dummy, 4, 2 ** 31 - 1, dummy, dummy, dummy, None)
    assert rc == -1 and b'n_vertices' in lib.psn_last_error()
    rc = lib.psn_cc_label(dummy, -1, 4, dummy, dummy, dummy, None)
    assert rc == -1 and b'n_faces' in lib.psn_last_error()
    rc = lib.psn_cc_label(dummy, 4, 4, dummy, dummy, None, None)
    assert rc == -1 and b'status' in lib.psn_last_error()
    rc = lib.psn_cc_label(None, 4, 4, dummy, dummy, dummy, None)
    assert rc == -1 and b'null pointer' in lib.psn_last_error()
    rc = lib.psn_cc_label(dummy, 4, 4, dummy, None, dummy, None)
    assert rc == -1 and b'null pointer' in lib.psn_last_error()
    rc = lib.psn_cc_stats(dummy, dummy, 4, 4, dummy, dummy, None, dummy, dummy, None)
    assert rc == -1 and b'null pointer' in lib.psn_last_error()
    rc = lib.psn_cc_flag(dummy, 4, 4, dummy, None, dummy, dummy, None)
    assert rc == -1 and b'null pointer' in lib.psn_last_error()
    args = (dummy, 4, 4, dummy, dummy, dummy, dummy)
    rc = lib.psn_cc_compact(dummy, None, 0, *args, 5, 1, dummy, None, dummy, None)
    assert rc == -1 and b'5 of 4 faces' in lib.psn_last_error()
    rc = lib.psn_cc_compact(dummy, None, 3, *args, 1, 1, dummy, None, dummy, None)
    assert rc == -1 and b'normal_bytes' in lib.psn_last_error()
    rc = lib.psn_cc_compact(dummy, None, 4, *args, 1, 1, dummy, None, dummy, None)
    assert rc == -1 and b'do not agree' in lib.psn_last_error()
    rc = lib.psn_cc_compact(dummy, dummy, 8, *args, 1, 1, dummy, None, dummy, None)
    assert rc == -1 and b'null pointer' in lib.psn_last_error()
    # the wrappers refuse host tensors like every other product path
    with pytest.raises(RuntimeError):
        hip.cc_label(torch.zeros(1, 3, dtype=torch.int64), 3, torch.zeros(1, dtype=torch.int32))
