"""mesheval.evaluate_mesh on the device against the host path from an equal rng state.  Every integer must be equal -- the precision and
recall counts, the inside and open counts, and with them iou, fscore, precision and recall exactly; the means agree within 1e-12
relative, the project's float64 gate (the device sums in another order)."""
import numpy as np
import pytest
import torch

from tests import inside_cases as ic
from tests import raycast_cases as rc
from psnerf_amd.mesheval import evaluate_mesh
from psnerf_amd.stage1.extracting import Mesh

pytestmark = pytest.mark.gpu
GATE = 1e-12
EXACT = ('thresholds', 'precision_count', 'recall_count', 'precision', 'recall', 'fscore', 'inside_pred', 'inside_gt', 'intersection', 'union',
         'n_open_pred', 'n_open_gt', 'open_pred', 'open_gt', 'iou', 'volume_pred', 'volume_gt', 'num_samples', 'iou_points')
MEANS = ('accuracy', 'completeness', 'chamfer', 'accuracy2', 'completeness2', 'chamfer2', 'normals_accuracy', 'normals_completeness', 'normals')


def cases(name):
    if name == 'two marching-cubes spheres':
        return Mesh(*ic.mc_sphere_small()[:2]), Mesh(*ic.mc_sphere()[:2]), {'thresholds': (0.5, 1.28, 1.3, 1.32, 3.0)}
    return Mesh(*rc.icosphere(2)), Mesh(*ic.hemisphere(2)), {}


@pytest.mark.parametrize('name', ['two marching-cubes spheres', 'hemisphere as ground truth'])
@pytest.mark.parametrize('vote', [False, True])
def test_device_equals_host(cuda, name, vote):
    from psnerf_amd import ops
    pred, gt, kw = cases(name)
    host = evaluate_mesh(pred, gt, 2000, iou_points=4000, rng=np.random.RandomState(7), vote=vote, **kw)
    ops.reset_hits()
    with ops.strict():
        dev = evaluate_mesh(pred, gt, 2000, iou_points=4000, rng=np.random.RandomState(7), vote=vote, device=cuda, **kw)
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    assert all(torch.is_tensor(x) and x.is_cuda for x in dev['raw'].values())
    print('%s: chamfer %.6g, iou %.4f, inside %d / %d, open %d / %d, normals %.4f' % (name, host['chamfer'], host['iou'], host['inside_pred'],
                                                                                   host['inside_gt'], host['n_open_pred'], host['n_open_gt'],
                                                                                   host['normals']))
    assert set(dev) == set(host)
    for key in EXACT:
        assert dev[key] == host[key], key
    for key in MEANS:
        print('    %s: %.17g / %.17g' % (key, dev[key], host[key]))
        assert abs(dev[key] - host[key]) <= GATE * abs(host[key]), key
    assert np.array_equal(dev['raw']['inside_gt'].cpu().numpy(), host['raw']['inside_gt'])
    assert 0 < host['inside_gt'] and 0.0 < host['iou'] < 1.0 and 0.0 < host['fscore'][host['thresholds'][2]]
    if name == 'hemisphere as ground truth':
        assert host['n_open_gt'] > 0 and host['n_open_pred'] == 0
    else:
        assert host['n_open_gt'] == 0 and host['n_open_pred'] == 0
