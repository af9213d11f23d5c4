"""mesheval.evaluate_mesh on the host path, and tools/evaluate_mesh.py over it."""
import json

import numpy as np

from tests import inside_cases as ic
from tests import raycast_cases as rc
from psnerf_amd import meshdist as md
from psnerf_amd import metrics
from psnerf_amd.mesheval import evaluate_mesh
from psnerf_amd.stage1.extracting import Mesh

N_SAMPLES, N_IOU = 1500, 6000     # x 320 faces: the brute-force host path stays under a second per query


def test_a_mesh_against_itself():
    mesh = Mesh(*rc.icosphere(2))
    out = evaluate_mesh(mesh, mesh, N_SAMPLES, iou_points=N_IOU, rng=np.random.RandomState(0))
    for key in ('accuracy', 'completeness', 'chamfer', 'accuracy2', 'completeness2', 'chamfer2'):
        assert abs(out[key]) <= 1e-15, key                      # (a sample lies on its own face up to the rounding of its barycentric sum)
    diagonal = float(np.linalg.norm(mesh.vertices.max(0) - mesh.vertices.min(0)))
    assert out['thresholds'] == [0.005 * diagonal, 0.01 * diagonal, 0.02 * diagonal]
    for t in out['thresholds']:
        assert out['fscore'][t] == 1.0 and out['precision'][t] == 1.0 and out['recall'][t] == 1.0
        assert out['precision_count'][t] == N_SAMPLES and out['recall_count'][t] == N_SAMPLES
    for key in ('normals', 'normals_accuracy', 'normals_completeness'):
        assert abs(out[key] - 1.0) <= 1e-12, key
    assert out['iou'] == 1.0 and out['inside_pred'] == out['inside_gt'] == out['intersection'] == out['union'] > 0
    assert out['open_pred'] == 0.0 and out['open_gt'] == 0.0 and out['n_open_pred'] == 0 and out['n_open_gt'] == 0


def test_chamfer_is_get_chamfer_dist_and_counts_follow_raw():
    pred, gt = Mesh(*ic.mc_sphere_small()[:2]), Mesh(*ic.mc_sphere()[:2])
    thresholds = (0.5, 1.28, 1.3, 1.32, 3.0)                     # lattice units; the radii differ by 1.29, the distances spread by 0.1
    out = metrics.evaluate_mesh(pred, gt, N_SAMPLES, thresholds=thresholds, iou_points=0, rng=np.random.RandomState(5))
    chamfer, raw = md.get_chamfer_dist(pred, gt, N_SAMPLES, rng=np.random.RandomState(5))
    assert out['chamfer'] == chamfer
    assert np.array_equal(out['raw']['pred_gt_dist'], raw['src_tgt_dist']) and np.array_equal(out['raw']['gt_pred_dist'], raw['tgt_src_dist'])
    assert out['accuracy'] == float(raw['src_tgt_dist'].mean()) and out['completeness'] == float(raw['tgt_src_dist'].mean())
    assert out['accuracy2'] == float((raw['src_tgt_dist'] ** 2).mean()) and out['chamfer2'] == (out['accuracy2'] + out['completeness2']) / 2
    assert out['thresholds'] == list(thresholds)
    seen = set()
    for t in thresholds:
        n_p, n_r = int((raw['src_tgt_dist'] <= t).sum()), int((raw['tgt_src_dist'] <= t).sum())
        assert out['precision_count'][t] == n_p and out['recall_count'][t] == n_r
        p, r = n_p / N_SAMPLES, n_r / N_SAMPLES
        assert out['precision'][t] == p and out['recall'][t] == r
        assert out['fscore'][t] == (2 * p * r / (p + r) if p + r > 0 else 0.0)
        seen.add((n_p, n_r))
    assert out['fscore'][0.5] == 0.0 and out['fscore'][3.0] == 1.0 and len(seen) == 5
    assert 0.9 < out['normals'] <= 1.0                           # concentric spheres: the closest triangle faces the same way
    # iou_points = 0 skips the block
    assert out['iou_points'] == 0 and not any(k in out for k in ('iou', 'inside_pred', 'volume_gt', 'open_pred'))


def test_iou_of_a_scaled_sphere_is_the_ratio_of_the_volumes():
    v, f = rc.icosphere(2)
    n = 20000
    out = evaluate_mesh(Mesh(0.5 * v, f), Mesh(v, f), 200, iou_points=n, rng=np.random.RandomState(9))
    box = float(np.prod(v.max(0) - v.min(0)))
    vol_small, vol = ic.volume(0.5 * v, f), ic.volume(v, f)
    assert abs(vol_small / vol - 0.125) < 1e-12
    # IoU = inside_pred / inside_gt here (the small sphere lies inside the large one); each count is a binomial share of the box
    assert out['intersection'] == out['inside_pred'] and out['union'] == out['inside_gt']
    assert abs(out['volume_pred'] - vol_small) <= ic.five_sigma(vol_small / box, n, box)
    assert abs(out['volume_gt'] - vol) <= ic.five_sigma(vol / box, n, box)
    # given the points inside gt, each is inside pred with probability 1 / 8: 5 sigma of that share
    m = out['inside_gt']
    assert abs(out['iou'] - vol_small / vol) <= 5.0 * np.sqrt(0.125 * 0.875 / m)
    assert out['open_pred'] == 0.0 and out['open_gt'] == 0.0


def test_hemisphere_as_ground_truth_is_reported_open():
    v, f = rc.icosphere(2)
    out = evaluate_mesh(Mesh(v, f), Mesh(*ic.hemisphere(2)), 300, iou_points=3000, rng=np.random.RandomState(2))
    voted = evaluate_mesh(Mesh(v, f), Mesh(*ic.hemisphere(2)), 300, iou_points=3000, rng=np.random.RandomState(2), vote=True)
    assert out['open_pred'] == 0.0 and out['open_gt'] > 0.3 and voted['open_gt'] == out['open_gt']
    assert voted['inside_pred'] == out['inside_pred'] and voted['inside_gt'] < out['inside_gt']
    assert out['recall'][out['thresholds'][0]] == 1.0 and out['precision'][out['thresholds'][0]] < 0.7


def test_the_tool(tmp_path, capsys):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('evaluate_mesh_tool', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                     'tools', 'evaluate_mesh.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pred_path, gt_path = str(tmp_path / 'pred.ply'), str(tmp_path / 'gt.ply')
    Mesh(*ic.mc_sphere_small()[:2]).export(pred_path)
    Mesh(*ic.mc_sphere()[:2]).export(gt_path)
    argv = [pred_path, gt_path, '--samples', '400', '--thresholds', '1.0', '2.0', '--iou-points', '1500', '--seed', '3', '--device', 'cpu']
    tool.main(argv + ['--json'])
    printed = json.loads(capsys.readouterr().out)
    want = evaluate_mesh(md.load_mesh(pred_path), md.load_mesh(gt_path), 400, thresholds=(1.0, 2.0), iou_points=1500, rng=np.random.RandomState(3))
    del want['raw']
    assert printed == json.loads(json.dumps(want))
    assert set(printed['fscore']) == {'1.0', '2.0'} and 0.0 < printed['iou'] < 1.0 and printed['open_gt'] == 0.0
    tool.main(argv)
    table = capsys.readouterr().out
    assert 'Chamfer distance' in table and 'F-score @ 1' in table and 'Volume IoU' in table
