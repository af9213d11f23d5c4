"""Vertex refinement on the device (psnerf_amd/stage1/extracting.py: one ops.GeoFieldFused call per step, d / dp from csrc/geo_dp.hip)
against the generic autograd form of the SAME definition on the oracle network, in float64 (truth) and float32 (the reference
arithmetic): the geometric-init BEAR network of tests/engine_cases.py and the mesh Extractor3D(resolution0=16, upsampling_steps=0)
extracts from it on the device.

Loss and gradient: the rule of tests/test_engines_gpu.py (bound = 1e-5 |truth| + 1e-5 max|truth| per tensor, the device allowed what
the float32 reference itself shows).  The loop: RMSprop normalises the step, so a coordinate whose gradient is at noise level moves
by +-1e-4 either way and an elementwise bound means nothing; with d(a, b) = mean |a - b| over coordinates the device must satisfy
d(device, host64) <= 2 d(host32, host64).

Measured on an MI355X (gfx950):
    the mesh: 408 faces (so the batches of 1000 and of all faces are the same 408), r_hip (r_ref) in units of the bound:
        1 face     loss 0.559 (0.323)   loss_target 7.051 (4.005)   loss_normal 0.034 (0.029)   dL/dv 1.950 (1.091)
        63 faces   loss 0.080 (0.243)   loss_target 0.144 (0.466)   loss_normal 0.008 (0.006)   dL/dv 0.459 (0.252)
        408 faces  loss 0.106 (0.293)   loss_target 0.177 (0.500)   loss_normal 0.006 (0.001)   dL/dv 0.093 (0.083)
    (the mesh IS the field's 0.5 level set, so loss_target = mean (occupancy - 0.5)^2 is a square of rounding-sized differences: on one
    face the float32 reference itself is 4 bounds off, and the device is held to twice that)
    the loop, 3 steps of 205 faces: d(device, host64) 1.586e-04   d(host32, host64) 1.586e-04   d(device, host32) 1.531e-09
    (on that level set the float64 and float32 gradients differ in sign on many coordinates, and RMSprop turns each into a full step;
    the device follows the float32 host run to 1.5e-9)
"""
import numpy as np
import pytest
import torch

from tests.helpers import assert_vs_truth, stage1_cfg, stage1_state_dict

pytestmark = pytest.mark.gpu
RTOL = 1e-5
_S = {}
_NOTES = []


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _NOTES:
        print('\n==== vertex refinement, device vs float64 ====')
        print('\n'.join(_NOTES))


def setup(cuda):
    """The device network, the oracle in float32 and float64 from one state dict, and the extracted mesh.  Built once."""
    if not _S:
        from oracle import stage1 as o1
        from psnerf_amd.stage1 import NeuralNetwork
        from psnerf_amd.stage1.extracting import Extractor3D
        cfg = stage1_cfg('bear')
        sd = stage1_state_dict(cfg, seed=21)
        net = NeuralNetwork(cfg)
        net.load_state_dict(sd)
        net = net.to(cuda).eval()
        oracles = {}
        for dtype in (torch.float32, torch.float64):
            o = o1.NeuralNetwork(cfg)
            o.load_state_dict(sd)
            oracles[dtype] = o.to(dtype).eval()
        mesh, _ = Extractor3D(net, device=cuda, resolution0=16, upsampling_steps=0).generate_mesh()
        assert 300 <= len(mesh.faces) <= 3000, len(mesh.faces)   # (408 on the sphere of the geometric initialisation)
        _S.update(net=net, oracles=oracles, mesh=mesh, v32=mesh.vertices.astype(np.float32))
    return _S


@pytest.mark.parametrize('n_faces', [1, 63, 1000, None], ids=lambda n: 'all' if n is None else str(n))
def test_refine_loss_and_vertex_gradient_vs_float64(cuda, n_faces):
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import refine_loss
    s = setup(cuda)
    F = len(s['mesh'].faces)
    n = F if n_faces is None else min(n_faces, F)
    rs = np.random.RandomState(100 + n)
    faces = torch.as_tensor(s['mesh'].faces[rs.permutation(F)[:n]])
    eps = torch.as_tensor(rs.dirichlet((0.5, 0.5, 0.5), size=n), dtype=torch.float32)

    def run(model, dtype, dev):
        v = torch.tensor(s['v32'], dtype=dtype, device=dev, requires_grad=True)
        terms = refine_loss(model, v, faces.to(dev), eps.to(dev, dtype), 0.5)
        terms[0].backward()
        return [t.detach().double().cpu().numpy().reshape(1) for t in terms] + [v.grad.double().cpu().numpy()]
    ops.reset_hits()
    with ops.strict():
        got = run(s['net'], torch.float32, cuda)
    assert ops.HITS['GeoFieldFused'] == 1 and not ops.FALLBACKS
    ref, truth = run(s['oracles'][torch.float32], torch.float32, 'cpu'), run(s['oracles'][torch.float64], torch.float64, 'cpu')
    assert np.abs(truth[3]).max() > 0
    for name, a, b, t in zip(('loss', 'loss_target', 'loss_normal', 'dL/dv'), got, ref, truth):
        rh, rr = assert_vs_truth('refine_loss %d faces: %s' % (n, name), a, b, t, RTOL, 'max')
        _NOTES.append('refine_loss %4d faces  %-12s r_hip %7.3f  r_ref %7.3f' % (n, name, rh, rr))


def test_refine_mesh_three_steps_across_an_epoch_vs_float64(cuda):
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D, refine_vertices
    s = setup(cuda)
    mesh, steps, seed = s['mesh'], 3, 7
    max_faces = len(mesh.faces) // 2 + 1   # two steps per epoch: step 3 opens the second one

    def device_run():
        ex = Extractor3D(s['net'], device=cuda, refine_max_faces=max_faces)
        ops.reset_hits()
        with ops.strict():
            out = ex.refine_mesh(mesh, steps=steps, rng=np.random.RandomState(seed))
        assert ops.HITS['GeoFieldFused'] == steps and not ops.FALLBACKS
        return out, ex.last_refine
    out, info = device_run()
    assert info['n_steps'] == steps and sorted(info) == ['loss_first', 'loss_last', 'n_steps', 'time (refine)']
    assert out.vertices.shape == mesh.vertices.shape and out.vertices.dtype == np.float64
    assert np.array_equal(out.faces, mesh.faces)
    moved = np.abs(out.vertices - s['v32'].astype(np.float64))
    assert 0.0 < moved.max() <= steps * 1e-4 * (1 + 1e-3)   # RMSprop: at most lr / sqrt(1 - alpha) per step
    again, _ = device_run()
    assert np.array_equal(again.vertices, out.vertices), 'two device runs from one seed differ'
    host = {}
    for dtype in (torch.float32, torch.float64):
        v, losses = refine_vertices(s['oracles'][dtype], s['v32'], mesh.faces, steps, max_faces, 0.5, np.random.RandomState(seed), 'cpu', dtype)
        assert len(losses) == steps
        host[dtype] = v.double().numpy()
    d = lambda a, b: float(np.abs(a - b).mean())
    d_dev, d_ref, d_dev32 = d(out.vertices, host[torch.float64]), d(host[torch.float32], host[torch.float64]), d(out.vertices, host[torch.float32])
    _NOTES.append('refine_mesh %d steps, %d faces / %d per step: d(device, host64) %.3e  d(host32, host64) %.3e  d(device, host32) %.3e'
                  % (steps, len(mesh.faces), max_faces, d_dev, d_ref, d_dev32))
    assert d_dev <= 2.0 * d_ref, (d_dev, d_ref)
