"""Mesh clean-up on the GPU (csrc/meshclean.hip through psnerf_amd/meshclean.py) against the numpy definition: labels and counts
exactly, areas within the rounding of a float64 sum, cleaned meshes bit for bit, two runs identical; then the extractor's new
arguments and the two command-line tools on the device.  The meshes (tests/meshclean_cases.py) are the smallest that still reach
every way the kernels can go wrong: empty inputs, one triangle, a long thin ribbon with shuffled ids (a deep union-find forest, a
duplicated face, a face with a repeated index, unreferenced vertices), two components, many components with a tie, many workgroups,
and a mesh whose ids and face order are shuffled so that a component's smallest index is not the first one met.

The labelling is a single pass (a lock-free union-find and a flatten launch): it has no rounds, so there is no round count to cap;
the ribbon would take neighbour-to-neighbour propagation 1734 rounds."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.helpers import ROOT
from tests import mesh_fields as mf
from tests.meshclean_cases import CASES, case
from psnerf_amd import meshclean as mc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def host(name):
    v, f = case(name)
    labels = mc.host_components(f, len(v))
    return labels, mc.host_component_table(v, f, labels)


def _assert_table(table, want, what):
    for key in ('label', 'n_vertices', 'n_faces'):
        assert table[key].dtype == np.int64 and np.array_equal(table[key], want[key]), '%s: %s' % (what, key)
    # Any summation order of n non-negative float64 terms is within (n - 1) 2^-53 relative of the exact sum, on each side; a factor 4
    # is left for last-bit differences per term: n_faces 2^-50 relative.
    gate = want['n_faces'] * 2.0 ** -50 * want['area']
    err = np.abs(table['area'] - want['area'])
    worst = float((err / np.maximum(gate, 1e-300)).max()) if len(err) else 0.0
    print('%s: %d components, worst area error %.3g of its gate' % (what, len(err), worst))
    assert table['area'].dtype == np.float64 and (err <= gate).all(), '%s: area' % what


def _same_mesh(a, b):
    return a.vertices.tobytes() == b.vertices.tobytes() and np.array_equal(a.faces, b.faces) and (
        (a.vertex_normals is None and b.vertex_normals is None) or a.vertex_normals.tobytes() == b.vertex_normals.tobytes())


def test_device_mover_takes_every_kind_of_input():
    """meshcore.device_mesh, which every device path starts with: nothing is launched but copies."""
    from psnerf_amd.meshcore import device_mesh
    tet_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)
    frozen_v, frozen_f = np.frombuffer(tet_v.tobytes(), dtype=np.float64).reshape(4, 3), np.frombuffer(tet_f.tobytes(), dtype=np.int64).reshape(4, 3)
    assert not frozen_v.flags.writeable and not frozen_f.flags.writeable
    placed = device_mesh(tet_v, tet_f, device=DEV)
    forms = [placed[:2], device_mesh(frozen_v, frozen_f, device=DEV)[:2],
             device_mesh(torch.from_numpy(tet_v).float(), torch.from_numpy(tet_f).int(), device=DEV)[:2], device_mesh(placed[0], placed[1])[:2],
             device_mesh(placed[0], placed[1], device=DEV)[:2]]
    for v, f in forms:
        assert v.is_cuda and f.is_cuda and v.dtype == torch.float64 and f.dtype == torch.int64 and v.is_contiguous() and f.is_contiguous()
        assert v.shape == (4, 3) and f.shape == (4, 3) and torch.equal(v, placed[0]) and torch.equal(f, placed[1])
    assert np.array_equal(placed[0].cpu().numpy(), tet_v) and np.array_equal(placed[1].cpu().numpy(), tet_f) and placed[2] is None
    for v, f in forms[3:]:                                                        # already in place: no copy
        assert v.data_ptr() == placed[0].data_ptr() and f.data_ptr() == placed[1].data_ptr()
    v, f, _ = device_mesh(tet_v, np.zeros((0, 3), dtype=np.int64), device=DEV)
    assert f.shape == (0, 3) and f.dtype == torch.int64 and f.is_cuda and v.shape == (4, 3)
    v, f, _ = device_mesh(np.zeros((0, 3)), [], device=DEV)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float64 and f.dtype == torch.int64
    n32 = np.arange(12, dtype=np.float32).reshape(4, 3)
    for normals in (n32, torch.from_numpy(n32), torch.from_numpy(n32).to(DEV)):
        kept = device_mesh(tet_v, tet_f, normals, device=DEV)[2]                   # meshclean's rule: the bits ride along
        wide = device_mesh(tet_v, tet_f, normals, device=DEV, widen_normals=True)[2]   # meshbake's rule
        assert kept.is_cuda and kept.dtype == torch.float32 and kept.cpu().numpy().tobytes() == n32.tobytes()
        assert wide.is_cuda and wide.dtype == torch.float64 and np.array_equal(wide.cpu().numpy(), n32)
    assert device_mesh(tet_v, tet_f, n32.astype(np.float16), device=DEV)[2].dtype == torch.float64    # neither float32 nor float64: widened
    with pytest.raises(ValueError, match=r'^atlas: 3 normals for 4 vertices'):
        device_mesh(tet_v, tet_f, n32[:3], device=DEV, prefix='atlas')


def test_degenerate_sizes():
    none_v, none_f = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    labels, table = mc.components(none_v, none_f, device=DEV)
    assert labels.dtype == torch.int32 and labels.shape == (0,) and all(len(table[k]) == 0 for k in table)
    mesh, report = mc.clean_mesh((none_v, none_f), device=DEV)
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and report['n_components'] == 0 and report['n_kept'] == 0
    five = np.random.RandomState(0).rand(5, 3)
    labels, table = mc.components(five, none_f, device=DEV)
    assert labels.cpu().tolist() == [0, 1, 2, 3, 4] and len(table['label']) == 0
    mesh, report = mc.clean_mesh((five, none_f), device=DEV)
    assert mesh.vertices.shape == (0, 3) and report['n_vertices_removed'] == 5 and report['n_faces_removed'] == 0
    tri = np.array([[4, 2, 3]])
    labels, table = mc.components(five, tri, device=DEV)
    assert labels.cpu().tolist() == [0, 1, 2, 2, 2]
    _assert_table(table, mc.host_component_table(five, tri, mc.host_components(tri, 5)), 'one triangle')
    mesh, report = mc.clean_mesh((five, tri), device=DEV)
    assert mesh.vertices.tobytes() == five[2:].tobytes() and mesh.faces.tolist() == [[2, 0, 1]] and report['n_vertices_removed'] == 2


@pytest.mark.parametrize('name', sorted(CASES))
def test_components_and_tables_against_the_definition(name):
    v, f = case(name)
    want_labels, want_table = host(name)
    dv, df = torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(f.copy()).to(DEV)
    labels, table = mc.components(dv, df)
    assert labels.dtype == torch.int32 and labels.is_cuda and np.array_equal(labels.cpu().numpy().astype(np.int64), want_labels)
    assert len(np.unique(want_labels)) == CASES[name]['classes']
    _assert_table(table, want_table, name)
    # two runs: identical labels and counts, identical cleaned meshes; and the cleaned mesh is the definition's
    labels2, table2 = mc.components(dv, df)
    assert torch.equal(labels, labels2) and all(np.array_equal(table[k], table2[k]) for k in ('label', 'n_vertices', 'n_faces'))
    first, report = mc.clean_mesh((dv, df), keep=1)
    second, _ = mc.clean_mesh((dv, df), keep=1)
    hv, hf, _, hreport = mc.host_clean(v, f, keep=1)
    assert _same_mesh(first, second) and first.vertices.tobytes() == hv.tobytes() and np.array_equal(first.faces, hf)
    assert all(report[k] == hreport[k] for k in ('n_components', 'n_kept', 'n_faces_removed', 'n_vertices_removed'))


@pytest.mark.parametrize('name,kw,normal_type', [('sphere_rod_torus', dict(keep=1), np.float32), ('checker16', dict(keep=2), np.float64),
                                                 ('checker32', dict(min_faces=16, keep=None), np.float32),
                                                 ('sphere_rod_torus', dict(keep=1, by='area'), None)])
def test_clean_mesh_against_host_clean(name, kw, normal_type):
    v, f = case(name)
    normals = None if normal_type is None else np.random.RandomState(7).randn(len(v), 3).astype(normal_type)
    hv, hf, hn, hreport = mc.host_clean(v, f, normals, **kw)
    mesh, report = mc.clean_mesh((v, f) if normals is None else (v, f, normals), device=DEV, **kw)
    assert mesh.vertices.dtype == np.float64 and mesh.vertices.tobytes() == hv.tobytes()
    assert mesh.faces.dtype == np.int64 and np.array_equal(mesh.faces, hf) and 0 < len(hf) < len(f)
    if normals is None:
        assert mesh.vertex_normals is None
    else:
        assert mesh.vertex_normals.dtype == normal_type and mesh.vertex_normals.tobytes() == hn.tobytes()
    assert all(report[k] == hreport[k] for k in ('n_components', 'n_kept', 'n_faces_removed', 'n_vertices_removed'))
    _assert_table(report['table'], hreport['table'], name)
    if name == 'checker16':   # the tie: two components of 16 faces, the smaller label stays
        t = hreport['table']
        assert (t['n_faces'] == 16).sum() == 2 and report['n_faces_removed'] == len(f) - 16212 - 16
        assert mc.select(report['table'], **kw).tolist() == mc.select(t, **kw).tolist()
    assert mf.is_closed_oriented(mesh.faces)


def test_extractor_on_the_device():
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D
    kw = dict(device=DEV, resolution0=16, upsampling_steps=2, points_batch_size=3000)
    with ops.strict():
        plain, pstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), **kw).generate_mesh()
        same, sstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), keep_components=None, min_component_faces=0, **kw).generate_mesh()
        ops.reset_hits()
        ex = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), keep_components=1, **kw)
        ex.phase_events = []
        kept, stats = ex.generate_mesh()
        assert ops.HITS['MeshComponents'] == 1 and not ops.FALLBACKS
    assert _same_mesh(plain, same) and sorted(pstats) == sorted(sstats) and 'n_components' not in sstats
    hv, hf, _, report = mc.host_clean(plain.vertices, plain.faces, keep=1)
    assert kept.vertices.tobytes() == hv.tobytes() and np.array_equal(kept.faces, hf) and len(hf) == 14656
    assert stats['n_components'] == 2 and stats['n_faces_removed'] == 8160 and stats['time (components)'] > 0.0
    assert 'components' in [name for name, _e0, _e1 in ex.phase_events]


def test_the_tools_end_to_end_on_the_device(tmp_path, capsys):
    """tools/extract_mesh.py --keep-components 1, then tools/chamfer_dist.py --keep-components 1 on what it wrote (in this process)."""
    import yaml
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.stage1 import NeuralNetwork
    from psnerf_amd.synthetic import stage1_cfg

    def tool(name):
        spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(ROOT, 'tools', name + '.py'))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        return module
    cfg = stage1_cfg('bear')
    cfg['extraction'] = {'resolution': 16, 'upsampling_steps': 1, 'refinement_step': 0}
    exp = tmp_path / 'out' / 'bear' / 'test_1'
    os.makedirs(str(exp / 'models'))
    with open(str(exp / 'config.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f)
    torch.manual_seed(0)
    CheckpointIO(str(exp / 'models'), model=NeuralNetwork(cfg)).save('model.pt')
    args = ['--obj_name', 'bear', '--exp_folder', str(tmp_path / 'out'), '--mesh_extension', 'obj']
    plain = tool('extract_mesh').main(args + ['--test_out_dir', str(tmp_path / 'a')])
    capsys.readouterr()
    kept = tool('extract_mesh').main(args + ['--test_out_dir', str(tmp_path / 'b'), '--keep-components', '1'])
    assert '1 connected components, 0 faces removed' in capsys.readouterr().out      # the sphere of the geometric initialisation
    assert open(plain).read() == open(kept).read()
    chamfer = tool('chamfer_dist').main(['--mesh_gt', plain, '--mesh_pred', kept, '--num_samples', '2000', '--seed', '0', '--keep-components', '1'])
    assert '1 of 1 connected components kept, 0 faces removed' in capsys.readouterr().out and 0.0 <= chamfer < 0.01
