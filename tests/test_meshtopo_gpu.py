"""Mesh connectivity on the GPU (csrc/meshtopo.hip through psnerf_amd/hip.py and psnerf_amd/meshtopo.py) against the numpy definition,
byte for byte: the edge table with its counters and vertex flags, the rings, the corner runs and both vertex-normal weights, on every
case of tests/meshtopo_cases.py; two runs give the same bytes; area and volume within the rounding of a float64 sum.  Every kernel
output lands in a buffer with guard zones on both sides (0xFF bytes) that must come back untouched."""
import numpy as np
import pytest
import torch

from tests import meshtopo_cases as tc
from psnerf_amd import meshocclude as mo, meshtopo as mt

pytestmark = pytest.mark.gpu
GUARD = 256


def dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)


def same_bits(t, a):
    """A device tensor and a numpy array of the same dtype hold the same bytes (NaN-safe, -0.0 is not +0.0)."""
    a = np.ascontiguousarray(a)
    h = t.cpu().numpy()
    return h.dtype == a.dtype and h.shape == a.shape and np.array_equal(h.reshape(-1).view(np.uint8), a.reshape(-1).view(np.uint8))


class Guarded(object):
    """``shape`` elements of ``dtype`` between two guard zones of 0xFF bytes."""

    def __init__(self, shape, dtype, cuda):
        n = int(np.prod(shape))
        self.raw = torch.full(((n + 2 * GUARD) * torch.empty(0, dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=cuda)
        self.all = self.raw.view(dtype)
        self.out = self.all[GUARD:GUARD + n].view(shape)

    def intact(self):
        n = self.out.numel()
        edge = torch.cat([self.all[:GUARD], self.all[GUARD + n:]]).contiguous().view(torch.uint8)
        return bool((edge == 0xFF).all())


def _edge_buffers(n_v, n_f, n_e, cuda):
    return [Guarded((n_e, 2), torch.int64, cuda), Guarded((n_e,), torch.int32, cuda), Guarded((n_e,), torch.int32, cuda),
            Guarded((3 * n_f,), torch.int64, cuda), Guarded((n_v,), torch.uint8, cuda), Guarded((n_v,), torch.uint8, cuda),
            Guarded((4,), torch.int64, cuda)]


@pytest.mark.parametrize('name', tc.NAMES)
def test_edge_table_rings_and_corner_runs_equal_the_definition(cuda, name):
    from psnerf_amd import hip
    v, f = tc.case(name)
    want, (want_start, want_ring), (want_corner_start, want_corner), want_report = tc.host(name)
    n_v, n_f, n_e = len(v), len(f), len(want['edges'])
    d_v, d_f = dev(v, cuda), dev(f, cuda)
    # ---- the edge table, into guarded buffers
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    keys = Guarded((3 * n_f,), torch.int64, cuda)
    assert same_bits(hip.topo_edge_keys(d_f, n_v, status, out=keys.out), mt.host_edge_keys(f, n_v)) and keys.intact() and int(status.item()) == 0
    bufs = _edge_buffers(n_v, n_f, n_e, cuda)
    got = mt._device_edges(d_f, n_v, out=tuple(b.out for b in bufs))
    assert got['n_edges'] == n_e and all(b.intact() for b in bufs)
    for key in ('edges', 'count', 'forward', 'halfedge_edge', 'counters'):
        assert same_bits(got[key], want[key]), '%s: %s' % (name, key)
    for key in ('vertex_used', 'vertex_open'):
        assert same_bits(got[key], want[key].astype(np.uint8)), '%s: %s' % (name, key)
    # ---- rings
    start, ring = Guarded((n_v + 1,), torch.int64, cuda), Guarded((2 * n_e,), torch.int64, cuda)
    got_start, got_ring = mt._device_rings(got['edges'], n_v, out=(start.out, ring.out))
    assert same_bits(got_start, want_start) and same_bits(got_ring, want_ring) and start.intact() and ring.intact()
    # ---- corner runs
    corner_start = Guarded((n_v + 1,), torch.int64, cuda)
    got_corner_start, got_corner = mt._device_corner_runs(d_f, n_v, out_start=corner_start.out)
    assert same_bits(got_corner_start, want_corner_start) and same_bits(got_corner, want_corner) and corner_start.intact()
    # ---- the public functions: the same, twice
    for _ in range(2):
        table = mt.edges((d_v, d_f))
        assert all(same_bits(table[k], got[k].cpu().numpy()) for k in got if k != 'n_edges')
        assert all(same_bits(a, b) for a, b in zip(mt.rings((d_v, d_f)), (want_start, want_ring)))
        assert all(same_bits(a, b) for a, b in zip(mt.corner_runs((v, f), device=cuda), (want_corner_start, want_corner)))


@pytest.mark.parametrize('name', tc.NAMES)
def test_vertex_normals_equal_the_definition(cuda, name):
    v, f = tc.case(name)
    d_v, d_f = dev(v, cuda), dev(f, cuda)
    for weight in ('area', 'uniform'):
        want = mt.host_vertex_normals(v, f, weight)
        out = Guarded((len(v), 3), torch.float64, cuda)
        got = mt._device_vertex_normals(d_v, d_f, weight, out=out.out)
        assert same_bits(got, want) and out.intact(), '%s, %s: %d rows differ' % (name, weight, int((got.cpu().numpy() != want).any(axis=1).sum()))
        assert same_bits(mt.vertex_normals((d_v, d_f), weight), want) and same_bits(mt.vertex_normals((v, f), weight, device=cuda), want)
    assert same_bits(mt.vertex_normals((d_v, d_f)), mo.area_weighted_normals(v, f))
    with pytest.raises(ValueError, match='weight'):
        mt.vertex_normals((d_v, d_f), 'angle')


@pytest.mark.parametrize('name', tc.NAMES)
def test_report_equals_the_definition(cuda, name):
    v, f = tc.case(name)
    want = tc.host(name)[3]
    d_v, d_f = dev(v, cuda), dev(f, cuda)
    got = mt.mesh_report((d_v, d_f))
    again = mt.mesh_report((v, f), device=cuda)
    assert got == again                                                                    # two runs: the same bits, the two sums included
    assert sorted(got) == sorted(want) and all(type(got[k]) is type(want[k]) for k in want)
    assert all(got[k] == want[k] for k in want if k not in ('area', 'volume'))
    # Any summation order of F float64 terms is within (F - 1) 2^-53 times the sum of their absolute values of the exact sum, on
    # each side; a factor 4 is left for last-bit differences per term (tests/test_meshclean_gpu.py:_assert_table): F 2^-50.
    out = torch.full((2 + 2 * GUARD,), float('nan'), dtype=torch.float64, device=cuda)
    sums = mt._device_measures(d_v, d_f, out=out[GUARD:GUARD + 2]).tolist()
    assert sums == [got['area'], got['volume']] and bool(torch.isnan(out[:GUARD]).all()) and bool(torch.isnan(out[GUARD + 2:]).all())
    terms = mt.host_measure_terms(v, f)
    for key, t in zip(('area', 'volume'), terms):
        gate = len(f) * 2.0 ** -50 * float(np.abs(t).sum())
        err = abs(got[key] - want[key])
        print('%s: %s %.17g, error %.3g of a gate of %.3g' % (name, key, got[key], err, gate))
        assert err <= gate, '%s: %s' % (name, key)


def test_out_of_range_indices_raise_on_the_device(cuda):
    v, f = tc.OUT_OF_RANGE
    d_v, d_f = dev(v, cuda), dev(f, cuda)
    for call in (lambda: mt.edges((d_v, d_f)), lambda: mt.mesh_report((d_v, d_f)), lambda: mt.rings((d_v, d_f)), lambda: mt.corner_runs((d_v, d_f)),
                 lambda: mt.vertex_normals((d_v, d_f)), lambda: mt.vertex_normals((v, f), device=cuda)):
        with pytest.raises(ValueError, match='a face refers to a vertex outside 0 .. 3'):
            call()
    none_v = torch.zeros(0, 3, dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError, match='a face refers to a vertex outside'):
        mt.edges((none_v, d_f))


def test_c_abi_refuses_bad_arguments(cuda):
    from psnerf_amd import hip
    v, f = tc.case('tet')
    d_v, d_f = dev(v, cuda), dev(f, cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        hip.topo_edge_keys(d_f.cpu(), 4, status)
    with pytest.raises(RuntimeError, match=r'faces \[F, 3\]'):
        hip.topo_edge_keys(d_f.reshape(-1), 4, status)
    with pytest.raises(RuntimeError, match='topo_runs'):
        hip.topo_runs(torch.zeros(4, dtype=torch.int64, device=cuda), 0, 4)
    with pytest.raises(RuntimeError, match='topo_edge_keys'):
        hip.topo_edge_keys(d_f, hip.CC_MAX_VERTICES + 1, status)
    ring_start, ring = mt.rings((d_v, d_f))
    with pytest.raises(RuntimeError, match='topo_smooth_step'):
        hip.topo_smooth_step(d_v, ring_start, ring, None, 0.5, out=d_v)                    # in place: refused
    with pytest.raises(RuntimeError, match='topo_smooth_step'):
        hip.topo_smooth_step(d_v, ring_start, ring, None, float('nan'))
    assert hip._lib.psn_topo_measures(d_v.data_ptr(), d_f.data_ptr(), 4, 4, None, None, None) == hip.E_ARG


def test_vertex_occlusion_without_normals_on_the_device(cuda):
    """vertex_occlusion of a device mesh without normals: the normals come from the kernel instead of the host, and every output
    equals the host path's, as the existing test demands of the call with normals."""
    from tests import raycast_cases as rc
    from psnerf_amd import ops
    v, f = rc.icosphere(2)
    f = f[:, ::-1].copy()                                       # inward normals, short rays: some directions blocked, some not
    host = mo.vertex_occlusion((v, f), K=16, t_max=0.3, bits=True)
    assert 0 < int(host[0].sum()) < 16 * len(v)
    ops.reset_hits()
    got = mo.vertex_occlusion((dev(v, cuda), dev(f, cuda)), K=16, t_max=0.3, bits=True)
    assert ops.HITS['MeshVertexNormals'] == 1
    assert all(x.is_cuda for x in got) and all(same_bits(a, b) for a, b in zip(got, host))
    by_name = mo.vertex_occlusion((v, f), K=16, t_max=0.3, bits=True, device=cuda)
    assert all(same_bits(a, b) for a, b in zip(by_name, host))
