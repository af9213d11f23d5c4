"""Vertex refinement (psnerf_amd/stage1/extracting.py: refine_loss, refine_vertices, Extractor3D.refine_mesh; tools/refine_mesh.py)
in its generic form on the host: an analytic field occupancy(p) = sigmoid(-10 (|p| - r)) -- the sphere of radius r at threshold 0.5 --
and a small icosphere built here."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from psnerf_amd.stage1.extracting import Extractor3D, Mesh, refine_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0.6


def icosphere(radius, subdivisions=2):
    """-> (vertices float64 [V, 3] on the sphere, faces int64 [F, 3] counter-clockwise seen from outside): 162 / 320 at 2."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    v, f = np.stack(v) * radius, np.array(f, dtype=np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 1]])
    assert (np.einsum('fc,fc->f', n, v[f].mean(1)) > 0).all()
    return v, f


class SphereField(object):
    """model(p [1, F, 3], None, only_occupancy=True) -> sigmoid(-10 (|p| - r)) [1, F, 1]; counts its calls."""

    def __init__(self, r):
        self.r, self.calls = r, 0

    def __call__(self, p, ray_d=None, only_occupancy=False, **kwargs):
        assert ray_d is None and only_occupancy
        self.calls += 1
        return torch.sigmoid(-10.0 * (p.norm(dim=-1, keepdim=True) - self.r))


def test_refine_loss_on_the_sphere_itself():
    v, f = icosphere(R)
    eps = np.random.RandomState(1).dirichlet((0.5, 0.5, 0.5), size=len(f))
    vt = torch.tensor(v, requires_grad=True)
    loss, loss_target, loss_normal = refine_loss(SphereField(R), vt, torch.tensor(f), torch.tensor(eps), 0.5)
    loss.backward()
    loss, loss_target, loss_normal = loss.detach(), loss_target.detach(), loss_normal.detach()
    fp = (v[f] * eps[:, :, None]).sum(1)
    occ = 1.0 / (1.0 + np.exp(10.0 * (np.linalg.norm(fp, axis=1) - R)))
    assert abs(float(loss_target) - float(((occ - 0.5) ** 2).mean())) <= 1e-14
    # flat faces against a curved field: the angle between a face's normal and the radial direction at a point of that face is at
    # most the face's angular radius (< 0.2 rad on this icosphere), and the squared chord of an angle a is 2 - 2 cos a <= a^2
    assert 0.0 < float(loss_normal) < 0.04
    assert float(loss) == float(loss_target + 0.01 * loss_normal)
    assert vt.grad is not None and bool(vt.grad.abs().sum() > 0)


def test_refine_mesh_pulls_an_inflated_icosphere_onto_the_surface():
    steps, max_faces = 20, 100
    v, f = icosphere(R + 0.02)
    normals = v / np.linalg.norm(v, axis=1, keepdims=True)
    mesh = Mesh(v, f, vertex_normals=normals)
    assert max_faces < len(f) and steps > -(-len(f) // max_faces)   # more than one epoch

    def run(seed):
        field = SphereField(R)
        ex = Extractor3D(field, device=torch.device('cpu'), refine_max_faces=max_faces, refinement_step=steps)
        out = ex.refine_mesh(mesh, rng=np.random.RandomState(seed))   # steps default to the constructor's refinement_step
        return out, ex.last_refine, field.calls

    out, info, calls = run(3)
    assert out is not mesh and np.array_equal(mesh.vertices, v)
    assert calls == steps and info['n_steps'] == steps
    assert sorted(info) == ['loss_first', 'loss_last', 'n_steps', 'time (refine)'] and info['loss_last'] < info['loss_first']
    dist = lambda x: float(np.abs(np.linalg.norm(x, axis=1) - R).mean())
    assert dist(out.vertices) < dist(v)
    # RMSprop: |step| = lr |g| / (sqrt(avg) + eps) with avg >= (1 - alpha) g^2, so at most lr / sqrt(1 - alpha) = 1e-5 / 0.1 per step; the
    # start is the float32 rounding of v
    moved = np.abs(out.vertices - v.astype(np.float32).astype(np.float64)).max()
    assert 0.0 < moved <= steps * 1e-4 * (1 + 1e-3)
    assert out.vertices.dtype == np.float64 and np.array_equal(out.vertices, out.vertices.astype(np.float32).astype(np.float64))
    assert np.array_equal(out.faces, f) and np.array_equal(out.vertex_normals, normals)
    again, _, _ = run(3)
    assert np.array_equal(again.vertices, out.vertices)
    other, _, _ = run(4)
    assert not np.array_equal(other.vertices, out.vertices)


def test_refine_mesh_returns_its_input_for_no_steps_and_for_an_empty_mesh():
    v, f = icosphere(R, 0)
    ex = Extractor3D(SphereField(R), device=torch.device('cpu'))
    mesh = Mesh(v, f)
    assert ex.refine_mesh(mesh) is mesh and ex.refine_mesh(mesh, steps=0) is mesh and ex.refine_mesh(mesh, steps=-1) is mesh
    empty = Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    assert ex.refine_mesh(empty, steps=5) is empty
    assert ex.model.calls == 0


def test_generate_mesh_still_refuses_the_constructor_argument_and_names_the_way():
    with pytest.raises(NotImplementedError, match='refinement_step.*refine_mesh'):
        Extractor3D(SphereField(R), device=torch.device('cpu'), resolution0=8, upsampling_steps=0, refinement_step=1).generate_mesh()


def test_refine_mesh_tool_on_the_host(tmp_path):
    """tools/refine_mesh.py --no-cuda: config.yaml + models/model.pt + a .ply in, the refined .ply out."""
    import yaml
    from oracle.stage1 import NeuralNetwork
    from psnerf_amd import meshdist
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.synthetic import stage1_cfg
    spec = importlib.util.spec_from_file_location('refine_mesh_tool', os.path.join(ROOT, 'tools', 'refine_mesh.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cfg = stage1_cfg('bear')
    cfg['extraction'] = {'resolution': 8, 'upsampling_steps': 1, 'refinement_step': 2}
    exp = tmp_path / 'out' / 'bear' / 'test_1'
    os.makedirs(str(exp / 'models'))
    with open(str(exp / 'config.yaml'), 'w') as fh:
        yaml.safe_dump(cfg, fh)
    torch.manual_seed(0)
    CheckpointIO(str(exp / 'models'), model=NeuralNetwork(cfg)).save('model.pt')
    v, f = icosphere(0.62, 1)   # near the sphere of the geometric initialisation
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'refined' / 'out.ply')
    Mesh(v, f).export(src)
    args = ['--no-cuda', '--obj_name', 'bear', '--exp_folder', str(tmp_path / 'out'), '--mesh', src, '--out', dst, '--refine-max-faces', '50',
            '--seed', '5']
    assert tool.main(args) == dst   # 2 steps, from the config
    a, b = meshdist.load_mesh(src), meshdist.load_mesh(dst)
    assert np.array_equal(a.faces, b.faces) and a.vertices.shape == b.vertices.shape
    moved = np.abs(a.vertices - b.vertices).max()
    assert 0.0 < moved <= 2 * 1e-4 * (1 + 1e-3)
    assert tool.main(args + ['--steps', '0']) == dst
    assert np.array_equal(meshdist.load_mesh(dst).vertices, a.vertices)
