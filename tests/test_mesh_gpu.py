"""Mesh extraction on the GPU (csrc/mesh.hip through psnerf_amd/stage1/extracting.py): the kernels alone against the numpy host
path, the look-up field of tests/mesh_fields.py through the whole device pipeline against the reference's recorded results, a
sphere-initialised network under ops.strict() against the CPU oracle and against the host path run on the device's own values,
and the shipped extraction size (resolution 64, 3 upsampling steps: a 513^3 grid)."""
import hashlib
import json
import os
import time

import numpy as np
import pytest
import torch

from tests.helpers import ATOL_LOGIT, ATOL_NORMAL, GOLDEN, assert_close, stage1_cfg
from tests import mesh_fields as mf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _holes(n, seed):
    g = np.random.RandomState(seed)
    grid = g.randn(n, n, n).astype(np.float32)
    grid[g.rand(n, n, n) < 0.7] = np.nan
    grid[:, n // 2, :] = np.nan           # lines along x and z that are all holes (they are filled by the y pass, if at all)
    grid[0, :, 0] = np.nan                # holes at index 0 of the x and z lines, and a y line that is all holes
    grid[0, 0, :] = np.nan                # a z line of holes that no pass can fill
    grid[n - 1, n - 1, n - 1] = 1.5
    return grid


@pytest.mark.parametrize('n', [3, 17, 65, 21])
def test_grid_ffill_is_bit_exact(n):
    from psnerf_amd import hip
    from psnerf_amd.stage1.extracting import host_ffill
    grid = _holes(n, n)
    ref = host_ffill(grid.copy())
    out = hip.grid_ffill(torch.from_numpy(grid).to(DEV)).cpu().numpy()
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    assert out.view(np.int32).tobytes() == ref.view(np.int32).tobytes()


@pytest.mark.parametrize('n', [3, 17, 65, 21])
def test_marching_cubes_kernels_against_the_host_path(n):
    from psnerf_amd import hip
    from psnerf_amd.stage1.extracting import CORNERS, host_marching_cubes, to_world
    grid = mf.checker(n - 1, seed=n)
    v_ref, f_ref = host_marching_cubes(grid, 0.0)
    dgrid = torch.from_numpy(grid).to(DEV)
    v, f = hip.marching_cubes(dgrid, 0.0)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    if n >= 17:   # every one of the 256 cases occurs
        P = np.pad(grid.astype(np.float64), 1, 'constant', constant_values=-1e6) <= 0.0
        M = n + 1
        cube = sum(P[dx:dx + M, dy:dy + M, dz:dz + M].astype(np.int64) << c for c, (dx, dy, dz) in enumerate(CORNERS))
        assert len(np.unique(cube)) == 256
    assert f.dtype == np.int64 and v.dtype == np.float64 and np.array_equal(f, f_ref) and v.shape == v_ref.shape
    err = np.abs(v - v_ref).max()
    print('n=%d: %d vertices, %d faces, max vertex difference %.3e lattice units, bit-equal: %s' % (n, len(v), len(f), err, np.array_equal(v, v_ref)))
    assert err <= 1e-12
    vw, fw = hip.marching_cubes(dgrid, 0.0, 2.4)
    errw = np.abs(vw.cpu().numpy() - to_world(v_ref, n, 2.4)).max()
    print('n=%d: world units: max difference %.3e, bit-equal: %s' % (n, errw, errw == 0.0))
    assert errw <= 1e-12 * 2.4 / (n - 1) and np.array_equal(fw.cpu().numpy(), f_ref)


def _to_lattice(vertices, n, box=2.4):
    return (np.asarray(vertices) / box + 0.5) * (n - 1) + 1.0


def _device_lookup(R, res0, depth):
    from psnerf_amd.stage1.extracting import Extractor3D
    model = mf.LookupModel(mf.sphere_rod_torus(R))
    ex = Extractor3D(model, device=DEV, resolution0=res0, upsampling_steps=depth, points_batch_size=3000)
    mesh, stats = ex.generate_mesh()
    return ex, model, mesh, stats


def test_lookup_field_through_the_device_pipeline_r32():
    g = np.load(os.path.join(GOLDEN, 'mesh_mise_r32.npz'))
    ex, model, mesh, stats = _device_lookup(32, 8, 2)
    known = np.zeros((33, 33, 33), dtype=bool)
    known[g['known'][:, 0], g['known'][:, 1], g['known'][:, 2]] = True
    seen = model.seen.cpu().numpy()
    assert np.array_equal(seen > 0, known) and seen.max() == 1 and np.array_equal(ex.last_known.cpu().numpy(), known)
    assert stats['n_points_evaluated'] == model.n_points == int(known.sum())
    assert ex.last_grid.cpu().numpy().tobytes() == g['dense'].tobytes()
    mf.assert_same_surface(_to_lattice(mesh.vertices, 33), mesh.faces, g['vertices'], g['faces'].astype(np.int64), 'device R=32')
    print('device R=32: rounds %d, points %d' % (stats['n_rounds'], stats['n_points_evaluated']))


def test_lookup_field_through_the_device_pipeline_r64():
    d = json.load(open(os.path.join(GOLDEN, 'mesh_mise_r64.json')))
    ex, model, mesh, stats = _device_lookup(64, 16, 2)
    assert stats['n_points_evaluated'] == model.n_points == d['n_known'] and int(model.seen.max()) == 1
    assert hashlib.sha256(np.ascontiguousarray(ex.last_grid.cpu().numpy().astype('<f4')).tobytes()).hexdigest() == d['dense_sha256']
    lat = _to_lattice(mesh.vertices, 65)
    assert (len(mesh.vertices), len(mesh.faces)) == (d['n_vertices'], d['n_faces'])
    assert mf.edges_digest(lat) == d['edges_sha256'] and mf.is_closed_oriented(mesh.faces)
    area, vol = mf.area_volume(lat, mesh.faces)
    assert vol * d['signed_volume'] > 0 and abs(vol - d['signed_volume']) < d['n_faces'] and abs(area - d['area']) < d['n_faces']


@pytest.mark.parametrize('case', ['below', 'above', 'clip', 'no_upsampling'])
def test_device_pipeline_equals_the_host_path_on_the_edge_cases(case):
    """An all-below field (empty mesh), an all-above field (the closed box the padding produces), clip=True and
    upsampling_steps=0: the device pipeline returns what the host path returns."""
    from psnerf_amd.stage1.extracting import Extractor3D
    field = {'below': np.full((33, 33, 33), -1.0, dtype=np.float32), 'above': np.full((33, 33, 33), 1.0, dtype=np.float32),
             'clip': mf.sphere_rod_torus(32) + np.float32(6.0), 'no_upsampling': mf.sphere_rod_torus(32)}[case]
    kw = dict(resolution0=33, upsampling_steps=0) if case == 'no_upsampling' else dict(resolution0=8, upsampling_steps=2)
    hm, dm = mf.LookupModel(field), mf.LookupModel(field)
    host, hstats = Extractor3D(hm, **kw).generate_mesh(clip=case == 'clip')
    ex = Extractor3D(dm, device=DEV, **kw)
    mesh, stats = ex.generate_mesh(clip=case == 'clip')
    assert np.array_equal(mesh.faces, host.faces) and mesh.vertices.shape == host.vertices.shape
    assert np.abs(mesh.vertices - host.vertices).max() <= 1e-12 * 2.4 / 32 if len(host.vertices) else True
    assert stats['n_points_evaluated'] == hstats['n_points_evaluated'] == dm.n_points and stats['n_rounds'] == hstats['n_rounds']
    assert mesh.is_empty == (case == 'below') and mf.is_closed_oriented(mesh.faces)
    if case == 'clip':
        assert bool((ex.last_grid[:, :, :3] == -30.0).all())


def _networks(seed=0):
    import psnerf_amd.stage1 as s1
    from oracle import stage1 as o1
    cfg = stage1_cfg('bear')
    torch.manual_seed(seed)
    onet = o1.NeuralNetwork(cfg)
    net = s1.NeuralNetwork(cfg)
    net.load_state_dict(onet.state_dict())
    return net.to(DEV), onet


def _n_components(n_vertices, faces):
    """Connected components of the vertex graph of a mesh (label propagation)."""
    label = np.arange(n_vertices)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], axis=0)
    while True:
        m = np.minimum(label[e[:, 0]], label[e[:, 1]])
        new = label.copy()
        np.minimum.at(new, e[:, 0], m)
        np.minimum.at(new, e[:, 1], m)
        if np.array_equal(new, label):
            return len(np.unique(label))
        label = new


def test_network_extraction_strict_against_oracle_and_host_path():
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D, grid_points_host
    net, onet = _networks()
    ops.reset_hits()
    with ops.strict():
        ex = Extractor3D(net, device=DEV, resolution0=16, upsampling_steps=2, with_normals=True)
        mesh, stats = ex.generate_mesh()
        grid, known = ex.last_grid.cpu().numpy(), ex.last_known.cpu().numpy()
        mesh2, stats2 = Extractor3D(net, device=DEV, resolution0=16, upsampling_steps=2, with_normals=True).generate_mesh()
        # upsampling_steps = 0 (extracting.py:90-96): the points are formed on the host and uploaded; still the lean engine
        flat, fstats = Extractor3D(net, device=DEV, resolution0=33, upsampling_steps=0).generate_mesh()
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    assert fstats['n_points_evaluated'] == 33 ** 3 and len(flat.faces) > 500 and mf.is_closed_oriented(flat.faces)
    print('network R=64: %s; %d vertices, %d faces' % (stats, len(mesh.vertices), len(mesh.faces)))
    assert stats['n_points_evaluated'] == int(known.sum()) and len(mesh.faces) > 1000
    # two runs are bit-identical
    assert np.array_equal(mesh.vertices, mesh2.vertices) and np.array_equal(mesh.faces, mesh2.faces)
    assert np.array_equal(mesh.vertex_normals, mesh2.vertex_normals) and stats2['n_rounds'] == stats['n_rounds']
    # the values of the evaluated points against the oracle on the host
    idx = np.argwhere(known)
    p = grid_points_host(idx, 64, 2.4)
    with torch.no_grad():
        ref = onet(p.unsqueeze(0), None, return_logits=True).reshape(-1)
    assert_close(torch.from_numpy(grid[known]), ref, 1e-4, 'mesh extraction: -logit of the evaluated points', atol=ATOL_LOGIT)
    # the host path on the device's own values: same evaluated set, identical mesh
    host_model = mf.LookupModel(grid)
    hmesh, hstats = Extractor3D(host_model, resolution0=16, upsampling_steps=2).generate_mesh()
    assert np.array_equal(host_model.seen.numpy() > 0, known) and hstats['n_points_evaluated'] == stats['n_points_evaluated']
    assert hstats['n_rounds'] == stats['n_rounds']
    assert np.array_equal(hmesh.faces, mesh.faces)
    err = np.abs(hmesh.vertices - mesh.vertices).max() if len(mesh.vertices) else 0.0
    print('device mesh vs host path on the same values: max vertex difference %.3e (world units), bit-equal: %s' % (err, err == 0.0))
    assert err <= 1e-12 * 2.4 / 64
    assert mf.is_closed_oriented(mesh.faces)
    # normals: -gradient / |gradient| of the oracle at the (float32) vertices
    pv = torch.as_tensor(mesh.vertices, dtype=torch.float32)
    g = onet.gradient(pv.unsqueeze(0), tflag=False).reshape(-1, 3)
    nref = -g / torch.norm(g, dim=-1, keepdim=True)
    assert_close(torch.from_numpy(mesh.vertex_normals), nref, 1e-4, 'mesh extraction: vertex normals', atol=ATOL_NORMAL)


def test_shipped_extraction_size_513():
    """resolution 64, upsampling_steps 3 (every shipped config): closed, consistently oriented; F = 2 V - 4 if the surface is one
    component of genus 0 (a sphere-initialised network: asserted only when the host path at a smaller size finds one component);
    inside the test's own time limit."""
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D
    net, _ = _networks()
    with ops.strict():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.time()
        ex = Extractor3D(net, device=DEV, resolution0=64, upsampling_steps=3)
        mesh, stats = ex.generate_mesh()
        dt = time.time() - t0
    peak = torch.cuda.max_memory_allocated() / 2.0 ** 20
    print('513^3: %.2f s, %s, %d vertices, %d faces, peak device memory %.0f MiB' % (dt, stats, len(mesh.vertices), len(mesh.faces), peak))
    assert dt < 120.0
    assert ex.last_grid.shape == (513, 513, 513) and stats['n_points_evaluated'] < 0.2 * 513 ** 3
    assert len(mesh.faces) > 100000 and mf.is_closed_oriented(mesh.faces)
    assert int(mesh.faces.max()) == len(mesh.vertices) - 1 and len(np.unique(mesh.faces)) == len(mesh.vertices)
    # Euler characteristic: the host path on the small grid's values says how many components the surface has
    from psnerf_amd.stage1.extracting import host_marching_cubes
    sgrid = Extractor3D(net, device=DEV, resolution0=16, upsampling_steps=2)
    sgrid.generate_mesh()
    hv, hf = host_marching_cubes(sgrid.last_grid.cpu().numpy(), 0.0)
    n_comp = _n_components(len(hv), hf)
    print('host path at 65^3: %d component(s), V = %d, F = %d' % (n_comp, len(hv), len(hf)))
    if n_comp == 1 and len(hf) == 2 * len(hv) - 4:
        assert len(mesh.faces) == 2 * len(mesh.vertices) - 4
    else:
        assert (len(mesh.faces) - 2 * len(mesh.vertices)) % 4 == 0   # F = 2 V - 4 (components - handles)
