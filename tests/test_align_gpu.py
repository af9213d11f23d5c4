"""Mesh registration on the GPU (csrc/meshalign.hip through psnerf_amd/hip.py and psnerf_amd/meshalign.py) against the float64 numpy
definition in the same module.  Outputs land in guarded buffers (NaN / 0xFF), so an element the kernel skips shows.

Gates, with where they come from:
  psn_align_transform, psn_align_dist   EQUAL, bit for bit: the kernels do the definition's float64 operations in the definition's
                        order with contraction off, and the square root is correctly rounded on both sides.
  psn_align_sums        the four counts EQUAL (integer counting of comparisons on bit-equal operands).  Each of the 37 sums within
                        n * 2^-50 * sum |term| of the definition: every term is formed bit for bit as the definition forms it; the
                        kernel and numpy add the same n signed terms in two different orders, each within n * 2^-53 * sum |term| of
                        the exact sum (the derivation of tests/test_ps_gpu.py, on absolute sums since the terms are signed).  Two
                        calls give the same bits.
  align_mesh            handed the host's transform of an iteration, the device's used count and max_dist EQUAL the host's (bit-equal
                        rows, an order statistic, exact counts).  Free-running, the CPU test's three gates: rotation <= 1e-10 degrees,
                        translation <= 1e-12 diag, scale <= 1e-12.
  evaluate_mesh(align)  chamfer within 1e-9 relative of the unmoved pair's, the issue's gate.
"""
import functools

import numpy as np
import pytest
import torch

from tests import align_cases as ac
from psnerf_amd import meshalign as ma
from psnerf_amd import mesheval

pytestmark = pytest.mark.gpu
GATES = (1e-10, 1e-12, 1e-12)     # degrees, fraction of the diagonal, scale
CHUNK = 1024                      # PSN_ALIGN_CHUNK


def dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)


def same_bits(t, a):
    """A device tensor and a numpy array of the same dtype hold the same bytes (NaN-safe, -0.0 is not +0.0)."""
    return np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8))


def guards(cuda):
    return (torch.full((37,), float('nan'), dtype=torch.float64, device=cuda), torch.full((4,), -1, dtype=torch.int64, device=cuda))


@functools.lru_cache(maxsize=None)
def host_rows(n, special=False):
    """One row set with its max_dist (the 0.9 order statistic of its finite distances) and the definition's result, computed once."""
    rows = ac.row_set(n, seed=n, special=special)
    d = ma.host_dist(rows['P'], rows['Y'])
    limit = ma._max_dist([d], 0.9, None)
    status, terms = ma.host_terms(rows['P'], rows['Y'], rows['tri'], rows['vertices'], rows['faces'], limit)
    sums, counts = ma.host_sums(rows['P'], rows['Y'], rows['tri'], rows['vertices'], rows['faces'], limit)
    for a in (rows['P'], rows['Y'], rows['tri'], rows['vertices'], rows['faces'], d, status, terms, sums, counts):
        a.setflags(write=False)
    return rows, d, limit, status, terms, sums, counts


def device_sums(cuda, rows, limit, rotation=None, out=None):
    from psnerf_amd import hip
    return hip.align_sums(dev(rows['P'], cuda), dev(rows['Y'], cuda), dev(rows['tri'], cuda), dev(rows['vertices'], cuda),
                          dev(rows['faces'], cuda), limit, rotation, out=out)


def check_sums(got, want, terms, n, what):
    bound = n * 2.0 ** -50 * np.abs(terms).sum(axis=0)
    err = np.abs(got - want)
    worst = int(np.argmax(err - bound))
    print('%s: n = %d, worst sum %d: |difference| %.3e against the bound %.3e' % (what, n, worst, err[worst], bound[worst]))
    assert np.isfinite(got).all() and (err <= bound).all(), (what, worst, err[worst], bound[worst])


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_transform_equals_the_definition_bit_for_bit(cuda, n):
    """Random points with planted denormals, -0.0, +0.0 and a huge value; two transforms, one of them with zeros in R so that -0.0
    products and sums occur."""
    from psnerf_amd import hip
    rng = np.random.RandomState(n)
    x = rng.standard_normal((n, 3))
    specials = [5e-324, -5e-324, 2.0 ** -1040, -0.0, 0.0, 1e300, -2.2250738585072014e-308]
    for i, s in enumerate(specials):
        x[(i * 7) % n, i % 3] = s
    K = ac.known(ac.STARTS[2], 3.0)
    transforms = [ma.from_matrix(K), (1.0, np.diag([1.0, -1.0, -1.0]), np.zeros(3)), (2.0 ** -30, np.eye(3), np.array([-0.0, 0.0, 5e-324]))]
    for s, R, t in transforms:
        want = ma.host_transform(x, s, R, t)
        out = torch.full((n, 3), float('nan'), dtype=torch.float64, device=cuda)
        got = hip.align_transform(dev(x, cuda), s, R, t, out=out)
        assert got is out and same_bits(got, want)
    y = x[::-1].copy()
    finite = np.where(np.abs(x) > 1e200, 1.0, x)
    d = hip.align_dist(dev(finite, cuda), dev(y, cuda), out=torch.full((n,), float('nan'), dtype=torch.float64, device=cuda))
    assert same_bits(d, ma.host_dist(finite, y))


@pytest.mark.parametrize('n', [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1])
def test_sums_at_every_size_teacher_forced(cuda, n):
    """Host-made rows in; one row below, at and above one workgroup's chunk and two chunks."""
    from psnerf_amd import hip
    assert hip.ALIGN_CHUNK == CHUNK and hip.ALIGN_SUMS == 37 and hip.ALIGN_COUNTS == 4
    rows, d, limit, status, terms, want, counts = host_rows(n)
    sums, cnt, partial = device_sums(cuda, rows, limit, out=guards(cuda))
    assert partial.numel() == 41 * ((n + CHUNK - 1) // CHUNK) == hip._lib.psn_align_workspace(n)
    assert cnt.tolist() == counts.tolist() and int(cnt.sum()) == n and counts[0] == ma.quantile_index(0.9, n) + 1
    check_sums(sums.cpu().numpy(), want, terms, n, 'align_sums')
    assert same_bits(hip.align_dist(dev(rows['P'], cuda), dev(rows['Y'], cuda)), d)


def test_sums_gating_ties_and_the_rotated_normal(cuda):
    """Rows with tri = -1, tri = F, a NaN in P, an inf in Y and a zero-area triangle land in their skip counts; max_dist set to one
    row's own distance keeps that row (closed test), the next smaller double drops it; the rotated-normal form against the
    definition."""
    n = 300
    rows, d, limit, status, terms, want, counts = host_rows(n, True)
    assert counts[1] == 4 and counts[2] == 1 and counts[3] > 0
    sums, cnt, _ = device_sums(cuda, rows, limit, out=guards(cuda))
    assert cnt.tolist() == counts.tolist()
    check_sums(sums.cpu().numpy(), want, terms, n, 'planted rows')
    tie = int(np.flatnonzero(status == 0)[7])
    args = (rows['P'], rows['Y'], rows['tri'], rows['vertices'], rows['faces'])
    for value, kept in ((float(d[tie]), True), (float(np.nextafter(d[tie], 0.0)), False)):
        st, tm = ma.host_terms(*args, value)
        assert (st[tie] == 0) == kept and (st[tie] == 3) != kept
        s2, c2, _ = device_sums(cuda, rows, value, out=guards(cuda))
        assert c2.tolist() == np.bincount(st, minlength=4).tolist()
        check_sums(s2.cpu().numpy(), tm[st == 0].sum(axis=0), tm, n, 'max_dist = a row\'s distance' if kept else 'just below it')
    R = ac.rotation(ac.AXIS, 37.0)
    st, tm = ma.host_terms(*args, limit, rotation=R)
    s3, c3, _ = device_sums(cuda, rows, limit, rotation=R, out=guards(cuda))
    assert c3.tolist() == np.bincount(st, minlength=4).tolist() == counts.tolist()
    check_sums(s3.cpu().numpy(), tm[st == 0].sum(axis=0), tm, n, 'rotated normal')
    assert np.abs(s3.cpu().numpy()[:28] - want[:28]).max() > 1e-3      # (the rotation is not ignored)
    # every row skipped: zero sums, not NaN
    s4, c4, _ = device_sums(cuda, dict(rows, tri=np.full(n, -1, dtype=np.int64)), limit, out=guards(cuda))
    assert c4.tolist() == [0, n, 0, 0] and not s4.cpu().numpy().any()


def test_sums_twice_give_the_same_bits(cuda):
    rows, d, limit = host_rows(2 * CHUNK + 1)[:3]
    a = device_sums(cuda, rows, limit, out=guards(cuda))
    b = device_sums(cuda, rows, limit)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'two runs differ'
    assert same_bits(a[0], b[0].cpu().numpy()) and same_bits(a[2], b[2].cpu().numpy())


@functools.lru_cache(maxsize=None)
def host_alignment(start_index, symmetric):
    """The host's run from a start of the table with its samples -> (K, source vertices, x, y, result)."""
    from psnerf_amd import meshdist
    v, f = ac.deformed_icosphere(2)
    K = ac.known(ac.STARTS[start_index], ac.diagonal(v))
    sv = ac.move(K, v)
    rng = np.random.RandomState(11)
    x = meshdist.host_sample_surface(sv, f, 400, rng)[0]
    y = meshdist.host_sample_surface(v, f, 400, rng)[0] if symmetric else None
    result = ma.align_mesh((sv, f), (v, f), mode='similarity', samples=400, symmetric=symmetric, init=None, rng=np.random.RandomState(11))
    return K, sv, x, y, result


@pytest.mark.parametrize('symmetric', [False, True])
def test_align_mesh_in_lock_step_and_free_running(cuda, symmetric):
    from psnerf_amd.meshdist import MeshIndex
    v, f = ac.deformed_icosphere(2)
    diag = ac.diagonal(v)
    tgt = MeshIndex(np.array(v), np.array(f), device=cuda)
    for start_index in range(3):
        K, sv, x, y, host = host_alignment(start_index, symmetric)
        src = MeshIndex(sv, np.array(f), device=cuda)
        if start_index == 1:      # lock step: the host's transform of every iteration in, its used count and max_dist out
            xd, yd = dev(x, cuda), (dev(y, cuda) if symmetric else None)
            for i, h in enumerate(host['history']):
                step = ma.align_step(src, tgt, xd, yd, h['transform'], keep=0.9, symmetric=symmetric)
                assert step['used'] == h['used'] and step['max_dist'] == h['max_dist'], (i, step['used'], h['used'], step['max_dist'], h['max_dist'])
                assert [int(c) for c in step['counts'][1:]] == h['skipped']
            assert len(host['history']) >= 5
        r = ma.align_mesh(src, tgt, mode='similarity', samples=400, symmetric=symmetric, init=None, rng=np.random.RandomState(11))
        err = ac.errors(r['matrix'], K, diag)
        print('device, start %s, symmetric %s: rotation %.3e deg, translation %.3e diag, scale %.3e; %d iterations (host %d), rms %.3e'
              % (ac.STARTS[start_index], symmetric, err[0], err[1], err[2], r['iterations'], host['iterations'], r['rms']))
        assert r['converged'] and all(e <= g for e, g in zip(err, GATES)), err
        assert r['used'] >= (720 if symmetric else 360) and r['rms'] <= 1e-14 * diag
    # the moments start and device tensors in place of an index
    K, sv, _, _, _ = host_alignment(2, symmetric)
    r = ma.align_mesh((dev(sv, cuda), dev(f, cuda)), (dev(v, cuda), dev(f, cuda)), mode='similarity', samples=400, symmetric=symmetric,
                      rng=np.random.RandomState(3))
    assert r['converged'] and all(e <= g for e, g in zip(ac.errors(r['matrix'], K, diag), GATES))


def test_evaluate_mesh_with_align_undoes_a_known_similarity(cuda):
    """What the feature is for.  The prediction is the ground truth with a dent (one vertex fan, under 3 % of the area, which keep =
    0.9 trims, so that the true transform stays an exact fixed point) and is handed over moved by a known similarity: align=None
    reports the misalignment, align='similarity' the Chamfer distance of the unmoved pair, from the same rng state."""
    v, f = ac.deformed_icosphere(2)
    diag = ac.diagonal(v)
    dented = np.array(v)
    dented[0] *= 0.8
    K = ac.known(ac.STARTS[1], diag)
    kw = dict(num_samples=4000, iou_points=2000, device='cuda')
    base = mesheval.evaluate_mesh((dented, f), (v, f), rng=np.random.RandomState(5), **kw)
    off = mesheval.evaluate_mesh((ac.move(K, dented), f), (v, f), rng=np.random.RandomState(5), **kw)
    got = mesheval.evaluate_mesh((ac.move(K, dented), f), (v, f), rng=np.random.RandomState(5), align='similarity', **kw)
    rel = abs(got['chamfer'] - base['chamfer']) / base['chamfer']
    print('chamfer: unmoved %.6e, moved %.6e, moved and aligned %.6e (relative difference %.3e); iou %.4f / %.4f / %.4f'
          % (base['chamfer'], off['chamfer'], got['chamfer'], rel, base['iou'], off['iou'], got['iou']))
    assert base['chamfer'] > 1e-5 * diag and off['chamfer'] > 5.0 * base['chamfer']
    assert rel <= 1e-9
    assert 'alignment' not in base and 'alignment' not in off
    a = got['alignment']
    assert a['converged'] and a['mode'] == 'similarity' and 'history' not in a
    assert all(e <= g for e, g in zip(ac.errors(a['matrix'], K, diag), GATES))
    assert got['iou'] == base['iou'] and off['iou'] < base['iou']
    moved = ma.apply(a['matrix'], (dev(ac.move(K, dented), cuda), dev(f, cuda)))
    assert np.array_equal(moved.faces, f) and np.abs(moved.vertices - dented).max() <= 1e-14 * diag


def test_entry_points_reject_bad_arguments(cuda):
    from psnerf_amd import hip
    rows, d, limit = host_rows(65)[:3]
    P, Y, tri, v, f = (dev(rows[k], cuda) for k in ('P', 'Y', 'tri', 'vertices', 'faces'))
    for bad in (float('nan'), -1.0, -float('inf')):
        with pytest.raises(RuntimeError, match='max_dist'):
            hip.align_sums(P, Y, tri, v, f, bad)
    hip.align_sums(P, Y, tri, v, f, float('inf'))
    import ctypes
    R, t = (ctypes.c_double * 9)(*np.eye(3).ravel()), (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    out = torch.empty(65, 3, dtype=torch.float64, device=cuda)
    part, sums, cnt = torch.empty(41, dtype=torch.float64, device=cuda), torch.empty(37, dtype=torch.float64, device=cuda), torch.empty(4, dtype=torch.int64, device=cuda)
    s = hip._stream()
    with pytest.raises(RuntimeError, match='align_transform: null pointer'):
        hip._check(hip._lib.psn_align_transform(None, 65, 1.0, R, t, out.data_ptr(), s), 'align_transform')
    with pytest.raises(RuntimeError, match='align_transform: null pointer'):
        hip._check(hip._lib.psn_align_transform(P.data_ptr(), 65, 1.0, None, t, out.data_ptr(), s), 'align_transform')
    with pytest.raises(RuntimeError, match='align_transform: n=-1'):
        hip._check(hip._lib.psn_align_transform(P.data_ptr(), -1, 1.0, R, t, out.data_ptr(), s), 'align_transform')
    with pytest.raises(RuntimeError, match='align_dist: null pointer'):
        hip._check(hip._lib.psn_align_dist(P.data_ptr(), None, 65, out.data_ptr(), s), 'align_dist')
    with pytest.raises(RuntimeError, match='align_dist: n=-5'):
        hip._check(hip._lib.psn_align_dist(P.data_ptr(), Y.data_ptr(), -5, out.data_ptr(), s), 'align_dist')
    with pytest.raises(RuntimeError, match='align_sums: null pointer'):
        hip._check(hip._lib.psn_align_sums(P.data_ptr(), Y.data_ptr(), None, 65, v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], None, 1.0,
                                           part.data_ptr(), sums.data_ptr(), cnt.data_ptr(), s), 'align_sums')
    with pytest.raises(RuntimeError, match='align_sums: null pointer'):
        hip._check(hip._lib.psn_align_sums(P.data_ptr(), Y.data_ptr(), tri.data_ptr(), 65, v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], None, 1.0,
                                           None, sums.data_ptr(), cnt.data_ptr(), s), 'align_sums')
    with pytest.raises(RuntimeError, match='align_sums: n=-1'):
        hip._check(hip._lib.psn_align_sums(P.data_ptr(), Y.data_ptr(), tri.data_ptr(), -1, v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], None, 1.0,
                                           part.data_ptr(), sums.data_ptr(), cnt.data_ptr(), s), 'align_sums')
    with pytest.raises(RuntimeError, match='faces'):
        hip._check(hip._lib.psn_align_sums(P.data_ptr(), Y.data_ptr(), tri.data_ptr(), 65, v.data_ptr(), v.shape[0], f.data_ptr(), 0, None, 1.0,
                                           part.data_ptr(), sums.data_ptr(), cnt.data_ptr(), s), 'align_sums')
    assert hip._lib.psn_align_workspace(-1) == -1 and hip._lib.psn_align_workspace(0) == 41
    assert hip._lib.psn_align_workspace(hip.ALIGN_MAX_ROWS + 1) == -1
    with pytest.raises(RuntimeError, match='float64'):
        hip.align_transform(P.float(), 1.0, np.eye(3), np.zeros(3))
    with pytest.raises(RuntimeError, match='rotation'):
        hip.align_transform(P, 1.0, np.eye(2), np.zeros(3))
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        hip.align_dist(P.cpu(), Y.cpu())
    with pytest.raises(RuntimeError, match='tri'):
        hip.align_sums(P, Y, tri[:10].contiguous(), v, f, 1.0)
    with pytest.raises(ValueError, match='both'):
        ma.align_mesh((v, f), (rows['vertices'], rows['faces']))
    empty = hip.align_sums(P[:0].contiguous(), Y[:0].contiguous(), tri[:0].contiguous(), v, f, 1.0, out=guards(cuda))
    assert empty[1].tolist() == [0, 0, 0, 0] and not empty[0].cpu().numpy().any()
