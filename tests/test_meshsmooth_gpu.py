"""Smoothing on the GPU (psn_topo_smooth_step through psnerf_amd/meshsmooth.py) against the numpy definition, byte for byte: the
positions after one step, after three lambda | mu pairs and after five plain Laplacian steps, with nothing, the boundary and a mask
pinned, on every case of tests/meshtopo_cases.py; two runs give the same bytes; then the extractor's new arguments on the device."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_fields as mf
from tests import meshtopo_cases as tc
from tests.test_meshtopo_gpu import Guarded, dev, same_bits
from psnerf_amd import meshsmooth as ms, meshtopo as mt

pytestmark = pytest.mark.gpu


def _mask(name):
    v, _ = tc.case(name)
    return np.random.RandomState(len(v)).rand(len(v)) < 0.3


@functools.lru_cache(maxsize=None)
def host(name, iterations, mu, pin):
    v, f = tc.case(name)
    return ms.host_smooth(v, f, iterations, 0.5, mu, _mask(name) if pin == 'mask' else pin)


@pytest.mark.parametrize('name', tc.NAMES)
def test_one_step_lands_in_a_guarded_buffer(cuda, name):
    from psnerf_amd import hip
    v, f = tc.case(name)
    table, (ring_start, ring), _, _ = tc.host(name)
    d_v = dev(v, cuda)
    d_start, d_ring = dev(ring_start, cuda), dev(ring, cuda)
    isolated = np.diff(ring_start) == 0
    for pinned in (None, table['vertex_open'], _mask(name)):
        held = isolated | (pinned if pinned is not None else False)
        for s in (0.5, -0.53):
            want = ms.host_step(v, ring_start, ring, held, s)
            out = Guarded((len(v), 3), torch.float64, cuda)
            got = hip.topo_smooth_step(d_v, d_start, d_ring, None if pinned is None else dev(pinned.astype(np.uint8), cuda), s, out=out.out)
            assert same_bits(got, want) and out.intact(), '%s, s = %g: %d rows differ' % (name, s, int((got.cpu().numpy() != want).any(axis=1).sum()))
    assert same_bits(d_v, v)                                                               # the input is never written


@pytest.mark.parametrize('name', tc.NAMES)
@pytest.mark.parametrize('iterations,mu,pin', [(1, -0.53, None), (3, -0.53, None), (3, -0.53, 'boundary'), (3, -0.53, 'mask'), (5, None, None)])
def test_smoothing_equals_the_definition(cuda, name, iterations, mu, pin):
    v, f = tc.case(name)
    want, want_report = host(name, iterations, mu, pin)
    d_v, d_f = dev(v, cuda), dev(f, cuda)
    pin_arg = _mask(name) if pin == 'mask' else pin
    got, report = ms._device_smooth(d_v, d_f, iterations, 0.5, mu, pin_arg)
    assert got.is_cuda and same_bits(got, want), '%s: %d rows differ' % (name, int((got.cpu().numpy() != want).any(axis=1).sum()))
    again, report2 = ms._device_smooth(d_v, d_f, iterations, 0.5, mu, dev(pin_arg, cuda) if pin == 'mask' else pin_arg)
    assert same_bits(again, want) and report2 == report and same_bits(d_v, v)
    assert all(report[k] == want_report[k] for k in ('n_pinned', 'n_isolated', 'iterations')) and type(report['n_pinned']) is int
    terms = (mt.host_measure_terms(v, f), mt.host_measure_terms(want, f))
    for when, (area, volume) in zip(('before', 'after'), terms):                           # report sums: the gate of test_meshtopo_gpu.py
        for key, t in (('area_', area), ('volume_', volume)):
            assert abs(report[key + when] - want_report[key + when]) <= len(f) * 2.0 ** -50 * float(np.abs(t).sum()), key + when
    # the displacement lengths are formed by the same operations on both paths, to a few units in the last place of the square root;
    # their mean is a sum of V terms in another order: (V - 1) 2^-53 of the sum of the terms, each at most the largest
    largest = want_report['max_displacement']
    assert abs(report['max_displacement'] - largest) <= 4 * 2.0 ** -52 * largest
    assert abs(report['mean_displacement'] - want_report['mean_displacement']) <= (4 + len(v)) * 2.0 ** -52 * largest


def test_smooth_mesh_on_the_device(cuda):
    from psnerf_amd import ops
    v, f = tc.case('sphere_rod_torus')
    ops.reset_hits()
    with ops.strict():
        mesh, report = ms.smooth_mesh((v, f), iterations=3, normals='area', device=cuda)
    assert ops.HITS['MeshSmooth'] == 1 and ops.HITS['MeshEdges'] == 1 and not ops.FALLBACKS
    want, _ = ms.host_smooth(v, f, 3)
    assert mesh.vertices.tobytes() == want.tobytes() and np.array_equal(mesh.faces, f)
    assert mesh.vertex_normals.tobytes() == mt.host_vertex_normals(want, f, 'area').tobytes()
    with pytest.raises(ValueError, match='a face refers to a vertex outside 0 .. 3'):
        ms.smooth_mesh(tc.OUT_OF_RANGE, device=cuda)
    with pytest.raises(ValueError, match='smooth: mu'):
        ms.smooth_mesh((v, f), mu=-0.5, device=cuda)


def _sphere():
    ax = np.arange(17, dtype=np.float64) / 16 - 0.5
    x, y, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    return (8.0 * (0.31 - np.sqrt((x + 0.03) ** 2 + (y - 0.02) ** 2 + (z + 0.01) ** 2))).astype(np.float32)


EXTRACT = dict(resolution0=17, upsampling_steps=0, points_batch_size=3000)


def test_extractor_on_the_device_equals_the_host_path(cuda):
    """Extractor3D(smooth_iterations=2) on the device equals the host path bytewise on a resolution-16 sphere (17 lattice points per
    axis, evaluated without upsampling)."""
    from psnerf_amd.stage1.extracting import Extractor3D
    host_plain, _ = Extractor3D(mf.LookupModel(_sphere()), device='cpu', **EXTRACT).generate_mesh()
    host_smooth, host_stats = Extractor3D(mf.LookupModel(_sphere()), device='cpu', smooth_iterations=2, **EXTRACT).generate_mesh()
    plain, _ = Extractor3D(mf.LookupModel(_sphere()), device=cuda, **EXTRACT).generate_mesh()
    smooth, stats = Extractor3D(mf.LookupModel(_sphere()), device=cuda, smooth_iterations=2, **EXTRACT).generate_mesh()
    print('unsmoothed: %d vertices, largest difference device - host %.3g; smoothed: %.3g' % (
        len(plain.vertices), np.abs(plain.vertices - host_plain.vertices).max(), np.abs(smooth.vertices - host_smooth.vertices).max()))
    assert len(smooth.faces) > 100 and smooth.faces.tobytes() == host_smooth.faces.tobytes() == plain.faces.tobytes()
    assert smooth.vertices.tobytes() == host_smooth.vertices.tobytes() != plain.vertices.tobytes()
    assert stats['n_vertices_pinned'] == host_stats['n_vertices_pinned'] == 0 and stats['smooth_iterations'] == host_stats['smooth_iterations'] == 2


def test_extractor_on_the_device(cuda):
    """With smooth_iterations=None nothing of the extraction changes; with a value the device tensors are smoothed between the
    marching cubes and the copy-back, and the result is the definition's on the unsmoothed extraction."""
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D
    sphere, kw = _sphere(), EXTRACT
    with ops.strict():
        plain, pstats = Extractor3D(mf.LookupModel(sphere), device=cuda, **kw).generate_mesh()
        ops.reset_hits()
        same, sstats = Extractor3D(mf.LookupModel(sphere), device=cuda, smooth_iterations=None, **kw).generate_mesh()
        assert 'MeshSmooth' not in ops.HITS and 'MeshEdges' not in ops.HITS
        ex = Extractor3D(mf.LookupModel(sphere), device=cuda, smooth_iterations=2, **kw)
        ex.phase_events = []
        smooth, stats = ex.generate_mesh()
        assert ops.HITS['MeshSmooth'] == 1 and not ops.FALLBACKS
    assert plain.vertices.tobytes() == same.vertices.tobytes() and plain.faces.tobytes() == same.faces.tobytes() and sorted(pstats) == sorted(sstats)
    want, report = ms.host_smooth(plain.vertices, plain.faces, 2)
    assert len(smooth.faces) > 100 and smooth.faces.tobytes() == plain.faces.tobytes()
    assert smooth.vertices.tobytes() == want.tobytes() != plain.vertices.tobytes()
    assert stats['smooth_iterations'] == 2 and stats['n_vertices_pinned'] == report['n_pinned'] == 0 and stats['time (smooth)'] > 0.0
    assert 'smooth' in [name for name, _e0, _e1 in ex.phase_events]
    assert mt.mesh_report(smooth)['is_oriented']
