"""Mesh simplification on the GPU (csrc/meshsimplify.hip through psnerf_amd/meshsimplify.py) against the numpy definition: clusters,
faces and every counter exactly, the vertices BIT FOR BIT (every operation is an IEEE basic operation in a stated order), two runs
identical; the face budget chooses the same grid through the same probes; errors come back through the status word; then the
extractor's new argument, the two command-line tools, and the sqrt(3) h bound through the device's own closest-point query.  The
meshes are tests/simplify_cases.py, the host results are computed once and shared (simplify_cases.host_result)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import ROOT
from tests import mesh_fields as mf
from tests.simplify_cases import RUNS, case, host_result, run_id
from psnerf_amd import meshsimplify as ms

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
COUNTERS = ('resolution', 'cell', 'dims', 'n_clusters', 'n_vertices', 'n_faces', 'n_clamped', 'n_faces_degenerate', 'n_faces_duplicate',
            'n_faces_flipped', 'probes')


def _device(name):
    v, f = case(name)
    return torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(f.copy()).to(DEV)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(ROOT, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.mark.parametrize('index', range(len(RUNS)), ids=[run_id(r) for r in RUNS])
def test_against_the_definition_bit_for_bit(index):
    name, kw = RUNS[index]
    v, f = case(name)
    want_v, want_f, want = host_result(index)
    dv, df = _device(name)
    grid = ms.make_grid(v.min(axis=0), v.max(axis=0), kw.get('cell'), kw.get('resolution'))
    cluster = ms._device_clusters(dv, grid)
    assert cluster.dtype == torch.int64 and np.array_equal(cluster.cpu().numpy(), ms.host_clusters(v, grid)[0])
    out_v, out_f, report = ms._device_simplify(dv, df, **kw)
    assert out_v.is_cuda and out_v.dtype == torch.float64 and out_f.dtype == torch.int64
    got_v, got_f = out_v.cpu().numpy(), out_f.cpu().numpy()
    assert got_v.shape == want_v.shape and got_f.shape == want_f.shape
    differ = int((got_v != want_v).sum())
    print('%s: %d clusters, %d vertices, %d faces; %d of %d coordinates differ from the definition' % (
        run_id(RUNS[index]), report['n_clusters'], len(got_v), len(got_f), differ, got_v.size))
    assert np.array_equal(got_f, want_f)
    assert all(report[k] == want[k] for k in COUNTERS), [(k, report[k], want[k]) for k in COUNTERS if report[k] != want[k]]
    assert got_v.tobytes() == want_v.tobytes()
    again_v, again_f, again = ms._device_simplify(dv, df, **kw)
    assert again_v.cpu().numpy().tobytes() == got_v.tobytes() and torch.equal(again_f, out_f) and all(again[k] == report[k] for k in COUNTERS)


@pytest.mark.parametrize('target', [200, 2000, 10000])
def test_target_faces_chooses_what_the_host_chooses(target):
    v, f = case('sphere')
    want_v, want_f, want = ms.host_simplify(v, f, target_faces=target)
    mesh, report = ms.simplify_mesh(_device('sphere'), target_faces=target)
    assert report['resolution'] == want['resolution'] and report['probes'] == want['probes'] and len(want['probes']) >= 12
    assert mesh.vertices.tobytes() == want_v.tobytes() and np.array_equal(mesh.faces, want_f) and 0 < len(mesh.faces) <= target
    assert all(report[k] == want[k] for k in COUNTERS)


def test_target_faces_unchanged_and_missed():
    v, f = case('cube16')
    mesh, report = ms.simplify_mesh((v, f), target_faces=len(f), device=DEV)
    assert report['unchanged'] is True and mesh.vertices.tobytes() == v.tobytes() and np.array_equal(mesh.faces, f)
    mesh, report = ms.simplify_mesh((v, f), target_faces=1, device=DEV)
    want_v, want_f, want = ms.host_simplify(v, f, target_faces=1)
    assert report['target_missed'] is True and report['probes'] == want['probes'] == [(ms.MAX_RESOLUTION, 3072), (1, 12)]
    assert mesh.vertices.tobytes() == want_v.tobytes() and np.array_equal(mesh.faces, want_f)


def test_errors_and_degenerate_sizes(monkeypatch):
    v, f = case('cube16')
    for index in (-1, len(v)):
        wrong = f.copy()
        wrong[100, 2] = index
        for kw in (dict(resolution=4), dict(target_faces=500)):
            with pytest.raises(ValueError, match='refers to a vertex outside'):
                ms.simplify_mesh((v, wrong), device=DEV, **kw)
    bad = v.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        ms.simplify_mesh((bad, f), resolution=4, device=DEV)
    for kw in (dict(), dict(cell=0.5, resolution=4), dict(cell=0.0), dict(resolution=ms.MAX_RESOLUTION + 1), dict(cell=1e-5)):
        with pytest.raises(ValueError):
            ms.simplify_mesh((v, f), device=DEV, **kw)
    monkeypatch.setattr(ms, 'MAX_CLUSTERS', 100)
    assert ms.simplify_mesh((v, f), resolution=4, device=DEV)[1]['n_clusters'] == 98
    with pytest.raises(ValueError, match='coarser cell'):
        ms.simplify_mesh((v, f), resolution=5, device=DEV)
    report = ms.simplify_mesh((v, f), target_faces=1000, device=DEV)[1]
    assert report['probes'] == ms.host_simplify(v, f, target_faces=1000)[2]['probes'] and report['probes'][0][1] == math.inf
    monkeypatch.undo()
    none_v, none_f = case('empty')
    for kw in (dict(resolution=3), dict(target_faces=5)):
        mesh, report = ms.simplify_mesh((none_v, none_f), device=DEV, **kw)
        assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and report['n_faces'] == 0
    with pytest.raises(ValueError):
        ms.simplify_mesh((none_v, np.array([[0, 1, 2]])), resolution=3, device=DEV)
    one = np.zeros((4, 3)) + 0.25                                   # zero extent on every axis: one cell with h = 1
    mesh, report = ms.simplify_mesh((one, np.array([[0, 1, 2], [1, 2, 3]])), resolution=7, device=DEV)
    assert report['cell'] == 1.0 and report['dims'] == (1, 1, 1) and report['n_clusters'] == 1 and report['n_faces_degenerate'] == 2
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3)


def test_extractor_on_the_device():
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D
    kw = dict(device=DEV, resolution0=16, upsampling_steps=2, points_batch_size=3000)
    with ops.strict():
        plain, pstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), **kw).generate_mesh()
        same, sstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), simplify_nfaces=None, **kw).generate_mesh()
        ops.reset_hits()
        ex = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), simplify_nfaces=3000, **kw)
        ex.phase_events = []
        small, stats = ex.generate_mesh()
        assert ops.HITS['MeshSimplify'] == 1 and not ops.FALLBACKS
    assert plain.vertices.tobytes() == same.vertices.tobytes() and np.array_equal(plain.faces, same.faces)
    assert sorted(pstats) == sorted(sstats) == ['n_points_evaluated', 'n_rounds', 'time (eval points)', 'time (marching cubes)']
    hv, hf, report = ms.host_simplify(plain.vertices, plain.faces, target_faces=3000)
    assert small.vertices.tobytes() == hv.tobytes() and np.array_equal(small.faces, hf) and 0 < len(hf) <= 3000 and small.vertex_normals is None
    assert stats['n_faces_simplified_from'] == len(plain.faces) == 22816 and stats['simplify_resolution'] == report['resolution']
    assert stats['time (simplify)'] > 0.0 and 'simplify' in [name for name, _e0, _e1 in ex.phase_events]
    # after the clean-up: the floaters go first, then the budget applies to what is left
    both, bstats = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(64)), keep_components=1, simplify_nfaces=3000, **kw).generate_mesh()
    from psnerf_amd import meshclean
    cv, cf, _, _ = meshclean.host_clean(plain.vertices, plain.faces, keep=1)
    hv, hf, _ = ms.host_simplify(cv, cf, target_faces=3000)
    assert both.vertices.tobytes() == hv.tobytes() and np.array_equal(both.faces, hf) and bstats['n_faces_simplified_from'] == 14656


def test_the_tools_end_to_end_on_the_device(tmp_path, capsys):
    """tools/simplify_mesh.py on a file written here; tools/extract_mesh.py --simplify-nfaces on a sphere-initialised model."""
    import yaml
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.meshdist import load_mesh
    from psnerf_amd.stage1 import NeuralNetwork
    from psnerf_amd.stage1.extracting import Mesh
    from psnerf_amd.synthetic import stage1_cfg
    v, f = case('cube16_rotated')
    Mesh(v, f).export(str(tmp_path / 'cube.obj'))
    path, report = _tool('simplify_mesh').main([str(tmp_path / 'cube.obj'), str(tmp_path / 'small.obj'), '--resolution', '9', '--device', 'cuda'])
    assert '3072 -> 482 faces' in capsys.readouterr().out
    written = load_mesh(path)
    want_v, want_f, want = host_result(RUNS.index(('cube16_rotated', dict(resolution=9))))
    assert written.vertices.tobytes() == want_v.tobytes() and np.array_equal(written.faces, want_f) and report['n_clamped'] == want['n_clamped']
    _, host_report = _tool('simplify_mesh').main([str(tmp_path / 'cube.obj'), str(tmp_path / 'host.obj'), '--target-faces', '500'])
    assert 0 < host_report['n_faces'] == len(load_mesh(str(tmp_path / 'host.obj')).faces) <= 500     # (the host path of the same tool)
    capsys.readouterr()

    cfg = stage1_cfg('bear')
    cfg['extraction'] = {'resolution': 16, 'upsampling_steps': 1, 'refinement_step': 0}
    exp = tmp_path / 'out' / 'bear' / 'test_1'
    os.makedirs(str(exp / 'models'))
    with open(str(exp / 'config.yaml'), 'w') as fh:
        yaml.safe_dump(cfg, fh)
    torch.manual_seed(0)
    CheckpointIO(str(exp / 'models'), model=NeuralNetwork(cfg)).save('model.pt')
    args = ['--obj_name', 'bear', '--exp_folder', str(tmp_path / 'out'), '--mesh_extension', 'obj']
    plain = load_mesh(_tool('extract_mesh').main(args + ['--test_out_dir', str(tmp_path / 'a')]))
    capsys.readouterr()
    small = load_mesh(_tool('extract_mesh').main(args + ['--test_out_dir', str(tmp_path / 'b'), '--simplify-nfaces', '300']))
    assert 'simplified from %d faces' % len(plain.faces) in capsys.readouterr().out
    hv, hf, _ = ms.host_simplify(plain.vertices, plain.faces, target_faces=300)
    assert 0 < len(small.faces) <= 300 < len(plain.faces) and small.vertices.tobytes() == hv.tobytes() and np.array_equal(small.faces, hf)


def test_vertices_stay_within_sqrt3_h_of_the_surface():
    """Every vertex of the simplified rotated cube lies within sqrt(3) h of the original surface (its cell holds an original vertex),
    measured by the device's own closest-point query."""
    from psnerf_amd.meshdist import MeshIndex
    index = MeshIndex(*_device('cube16_rotated'))
    for n in (4, 17):
        out_v, out_f, report = ms._device_simplify(*_device('cube16_rotated'), resolution=n)
        assert report['n_clamped'] > 0
        _, dist, _ = index.closest_point(out_v)
        worst = float(dist.max()) / report['cell']
        print('resolution %d: %d vertices, at most %.3f h from the original surface' % (n, len(out_v), worst))
        assert worst <= math.sqrt(3.0)


def test_the_cluster_limit_is_the_definition_s_error_when_the_kernel_meets_it_too(monkeypatch):
    """Beyond PSN_VC_MAX_CLUSTERS clusters the face-key kernel cannot pack some ids, skips those faces and sets PSN_VC_E_CLUSTER.  That
    order of events -- the kernel's own limit fires, THEN the caller looks at the count -- must end where the definition ends:
    ValueError ('coarser cell') for a fixed grid, +inf for a probe of the face budget.  Two million occupied cells are not needed to
    take it: the kernel is handed the cluster ids shifted up to its limit (the real kernel sets the real bit), and the Python
    limit is lowered so that the count exceeds it, as in the other limit tests."""
    from psnerf_amd import hip
    v, f = case('cube16')
    dv, df = _device('cube16')
    real, shift = hip.vc_face_keys, hip.VC_MAX_CLUSTERS - 50

    def shifted(faces, cluster, status, want_corners=True):
        out = real(faces, cluster + shift, status, want_corners)
        assert int(status.item()) & hip.VC_E_CLUSTER and int((out[1] >= 0).sum()) < int((real(faces, cluster, status.clone(), False)[1] >= 0).sum())
        return out
    # the kernel itself: ids at or above the limit set the bit, the face is skipped (key -1, g = 0), ids below it are packed
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    cluster = torch.arange(len(v), dtype=torch.int64, device=DEV) + (hip.VC_MAX_CLUSTERS - 3)
    tri = torch.tensor([[0, 1, 2], [2, 1, 0], [2, 3, 4]], dtype=torch.int64, device=DEV)
    _, keys, g = hip.vc_face_keys(tri, cluster, status, want_corners=False)
    low = hip.VC_MAX_CLUSTERS - 3
    assert int(status.item()) == hip.VC_E_CLUSTER and keys.tolist() == [(low << 42) + ((low + 1) << 21) + low + 2, (low << 42) + ((low + 2) << 21) + low + 1, -1]
    assert g.tolist() == [[low, low + 1, low + 2], [low + 2, low + 1, low], [0, 0, 0]]
    monkeypatch.setattr(hip, 'vc_face_keys', shifted)
    with pytest.raises(RuntimeError, match='cluster id outside'):          # within the limit the bit is a fault of the pipeline's own
        ms._device_simplify(dv, df, resolution=5)
    monkeypatch.setattr(ms, 'MAX_CLUSTERS', 100)
    with pytest.raises(ValueError, match='coarser cell'):                  # 152 clusters: the definition's error, not the status word's
        ms._device_simplify(dv, df, resolution=5)
    with pytest.raises(ValueError, match='coarser cell'):
        ms._device_simplify(dv, df, cell=0.4)
    wrong = df.clone()
    wrong[100, 2] = len(v)
    with pytest.raises(ValueError, match='refers to a vertex outside'):    # an index error still comes first, as on the host
        ms._device_simplify(dv, wrong, resolution=5)
    want = ms.host_simplify(v, f, target_faces=1000)[2]
    monkeypatch.setattr(hip, 'vc_face_keys', lambda faces, cluster, status, want_corners=True:
                        shifted(faces, cluster, status, want_corners) if int(cluster.max()) >= 100 else real(faces, cluster, status, want_corners))
    report = ms._device_simplify(dv, df, target_faces=1000)[2]
    assert report['probes'] == want['probes'] and report['probes'][0] == (ms.MAX_RESOLUTION, math.inf) and report['resolution'] == want['resolution']
    assert report['n_clusters'] <= 100 and 0 < report['n_faces'] <= 1000
