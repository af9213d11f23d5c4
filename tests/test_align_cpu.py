"""Mesh registration, the definition (psnerf_amd/meshalign.py: host_*): numpy only, no library needed.

Gates, with where they come from.  Source and target are the SAME mesh up to the known similarity, so at the true transform every
residual is zero and the true transform is a fixed point of the rule; Gauss-Newton on a zero-residual problem converges quadratically
(the issue's prototype: 6 - 7 iterations to rounding level), so what is left is float64 rounding of the closest points and of the
7 x 7 solve: rotation <= 1e-10 degrees, translation <= 1e-12 of the target's diagonal, scale <= 1e-12, the issue's gates, four orders
above the 1e-14 degrees, 4e-17 and 2e-16 that this definition reaches here.  The rotation error is measured from the skew part of
the residual rotation (align_cases.errors), not by an arccos, which is blind below 1e-8 rad.
"""
import inspect
import json
import os

import numpy as np
import pytest

from tests import align_cases as ac
from psnerf_amd import meshalign as ma
from psnerf_amd import mesheval, metrics
from psnerf_amd.meshcore import Mesh, load_mesh

GATES = (1e-10, 1e-12, 1e-12)     # degrees, fraction of the diagonal, scale


def target():
    v, f = ac.deformed_icosphere(2)
    return v, f, ac.diagonal(v)


def within_gates(result, K, diag, what):
    err = ac.errors(result['matrix'], K, diag)
    print('%s: rotation %.3e deg, translation %.3e diag, scale %.3e; %d iterations, converged %s, rms %.3e over %d rows'
          % (what, err[0], err[1], err[2], result['iterations'], result['converged'], result['rms'], result['used']))
    assert result['converged'] and all(e <= g for e, g in zip(err, GATES)), (what, err)
    return err


@pytest.mark.parametrize('start', ac.STARTS)
def test_the_three_starts_of_the_table_converge(start):
    """From the identity (init=None) and from the moments start, 400 samples, keep 0.9."""
    v, f, diag = target()
    K = ac.known(start, diag)
    for init in (None, 'moments'):
        r = ma.align_mesh((ac.move(K, v), f), (v, f), mode='similarity', samples=400, init=init, rng=np.random.RandomState(1))
        within_gates(r, K, diag, 'start %s init %s' % (start, init))
        assert r['iterations'] <= 10 and r['start'] is None and len(r['history']) == r['iterations']
        assert r['rms'] <= 1e-14 * diag and r['used'] >= ma.quantile_index(0.9, 400) + 1
        assert np.allclose(r['matrix'][:3, :3], r['scale'] * r['rotation'], rtol=0, atol=1e-15) and np.array_equal(r['matrix'][:3, 3], r['translation'])
        rms = [h['rms'] for h in r['history']]
        assert all(b < a for a, b in zip(rms, rms[1:])), rms      # monotone on this zero-residual problem
        assert all(sum(h['skipped']) + h['used'] == 400 and h['skipped'][0] == 0 and h['skipped'][1] == 0 for h in r['history'])


def test_symmetric_reaches_the_same_transform():
    v, f, diag = target()
    for start in ac.STARTS:
        K = ac.known(start, diag)
        r = ma.align_mesh((ac.move(K, v), f), (v, f), mode='similarity', samples=400, symmetric=True, init=None, rng=np.random.RandomState(2))
        within_gates(r, K, diag, 'symmetric, start %s' % (start,))
        assert all(sum(h['skipped']) + h['used'] == 800 for h in r['history'])


def test_rigid_on_a_scaled_copy_says_that_it_does_not_fit():
    """A copy scaled by 1.08 cannot be matched by a rigid motion: the surfaces stay about 0.08 x the mean radius apart on every side
    (about 0.02 of the diagonal), whatever the rotation and translation.  The gate is a quarter of that; the result must not claim
    a converged zero-residual fit, and the scale must be exactly 1."""
    v, f, diag = target()
    K = ac.known((0.0, 0.0, 1.08), diag)
    r = ma.align_mesh((ac.move(K, v), f), (v, f), mode='rigid', samples=400, max_iterations=20, rng=np.random.RandomState(1))
    print('rigid on a copy scaled by 1.08: rms %.4f diag, converged %s after %d iterations' % (r['rms'] / diag, r['converged'], r['iterations']))
    assert r['scale'] == 1.0 and r['rms'] > 0.005 * diag
    assert not (r['converged'] and r['rms'] < 1e-6 * diag)
    s = ma.align_mesh((ac.move(K, v), f), (v, f), mode='similarity', samples=400, rng=np.random.RandomState(1))
    assert s['converged'] and s['rms'] < 1e-14 * diag and abs(s['scale'] * 1.08 - 1.0) <= 1e-12


def test_translation_leaves_rotation_and_scale_alone():
    v, f, diag = target()
    K = ac.known((0.0, 0.03, 1.0), diag)
    r = ma.align_mesh((ac.move(K, v), f), (v, f), mode='translation', samples=400, init=None, rng=np.random.RandomState(1))
    assert np.array_equal(r['rotation'], np.eye(3)) and r['scale'] == 1.0
    err = within_gates(r, K, diag, 'translation')
    assert err[0] == 0.0 and err[2] == 0.0


def test_partial_overlap_with_keep_0_7():
    """A third of the source's faces removed, symmetric rows, keep = 0.7: measured on the CPU, 22 % of the target's samples have no
    counterpart on the partial source (11 % of all rows), so keep = 0.7 trims all of them.  Achieved from the 8 degree / 0.03 diag /
    1.04 start: rotation 7.9e-15 degrees, translation 1.9e-17 diag, scale 0 (keep = 0.9, which cannot trim 11 %, ends 9e-3 degrees
    off)."""
    v, f, diag = target()
    K = ac.known(ac.STARTS[1], diag)
    pv, pf = ac.without_a_third(ac.move(K, v), f)
    assert len(pf) == len(f) - len(f) // 3
    for symmetric in (True, False):
        r = ma.align_mesh((pv, pf), (v, f), mode='similarity', samples=400, keep=0.7, symmetric=symmetric, init=None, rng=np.random.RandomState(1))
        within_gates(r, K, diag, 'partial source, symmetric %s' % symmetric)
        assert r['used'] >= (560 if symmetric else 280)


def test_axes24_picks_the_right_start():
    """A copy turned by 90 degrees about x and 5 degrees more: the start that undoes the quarter turn has the lowest rms after the coarse
    stage, and the fine stage then meets the gates."""
    v, f, diag = target()
    quarter = ac.rotation([1.0, 0.0, 0.0], 90.0)
    K = np.eye(4)
    K[:3, :3] = ac.rotation(ac.AXIS, 5.0) @ quarter
    table = ma.axes24()
    assert len(table) == 24 and np.array_equal(table[0], np.eye(3))
    assert all(abs(np.linalg.det(R) - 1.0) < 1e-15 and np.array_equal(np.abs(R).sum(0), np.ones(3)) for R in table)
    assert len({R.tobytes() for R in table}) == 24
    want = [i for i, R in enumerate(table) if np.allclose(R, quarter.T, atol=1e-12)]
    r = ma.align_mesh((ac.move(K, v), f), (v, f), mode='rigid', samples=400, starts='axes24', coarse_samples=100, coarse_iterations=4,
                      rng=np.random.RandomState(1))
    assert [r['start']] == want
    within_gates(r, K, diag, 'axes24')


def test_apply_keeps_faces_and_rotates_normals():
    v, f, diag = target()
    normals = v / np.linalg.norm(v, axis=1, keepdims=True)
    K = ac.known(ac.STARTS[2], diag)
    out = ma.apply(K, Mesh(v, f, vertex_normals=normals))
    assert isinstance(out, Mesh) and np.array_equal(out.faces, f) and out.faces is not f
    assert np.allclose(out.vertices, ac.move(K, v), rtol=0, atol=1e-15)
    R = K[:3, :3] / 1.08
    assert np.allclose(out.vertex_normals, normals @ R.T, rtol=0, atol=1e-15)
    assert np.allclose(np.linalg.norm(out.vertex_normals, axis=1), 1.0, rtol=0, atol=1e-15)
    assert ma.apply(K, (v, f)).vertex_normals is None
    # the transform's stated operation order, element by element
    s, Rm, t = ma.from_matrix(K)
    x = v[5]
    want = [s * ((Rm[i, 0] * x[0] + Rm[i, 1] * x[1]) + Rm[i, 2] * x[2]) + t[i] for i in range(3)]
    assert ma.host_transform(x[None], s, Rm, t)[0].tolist() == want
    back = ma.host_transform(ma.host_transform(v, s, Rm, t), *ma.inverse((s, Rm, t)))
    assert np.abs(back - v).max() <= 1e-15


def test_a_reflection_is_refused():
    v, f, _ = target()
    mirror = np.diag([1.0, 1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match='reflection'):
        ma.apply(mirror, (v, f))
    with pytest.raises(ValueError, match='reflection'):
        ma.align_mesh((v, f), (v, f), init=mirror, samples=50)
    with pytest.raises(ValueError, match='no proper rotation'):
        ma.align_mesh((v, f), (v, f), starts=[np.diag([1.0, -1.0, 1.0])], samples=50)
    with pytest.raises(ValueError, match='not a scale times a rotation'):
        ma.apply(np.diag([1.0, 2.0, 1.0, 1.0]), (v, f))
    with pytest.raises(ValueError, match='mode'):
        ma.align_mesh((v, f), (v, f), mode='affine')
    with pytest.raises(ValueError, match='keep'):
        ma.align_mesh((v, f), (v, f), keep=0.0)
    with pytest.raises(ValueError, match='max_dist'):
        ma.align_mesh((v, f), (v, f), max_dist=float('nan'))


def test_gate_counts_quantile_and_ties_of_the_definition():
    rows = ac.row_set(40, seed=3, special=True)
    P, Y, tri, v, f = (rows[k] for k in ('P', 'Y', 'tri', 'vertices', 'faces'))
    d = ma.host_dist(P, Y)
    finite = np.where(np.isfinite(d), d, np.inf)
    assert ma.quantile_index(0.9, 40) == 35 and ma.quantile_index(1.0, 40) == 39 and ma.quantile_index(1e-9, 40) == 0
    limit = float(np.sort(finite)[ma.quantile_index(0.5, 40)])
    assert ma._max_dist([d[:11], d[11:]], 0.5, None) == limit and ma._max_dist([d], 0.5, 0.5 * limit) == 0.5 * limit
    status, terms = ma.host_terms(P, Y, tri, v, f, limit)
    planted = rows['planted']
    assert [int(status[planted[k]]) for k in ('no_triangle', 'beyond_last', 'nan_P', 'inf_Y', 'zero_area')] == [1, 1, 1, 1, 2]
    sums, counts = ma.host_sums(P, Y, tri, v, f, limit)
    others = np.ones(40, bool)
    others[list(planted.values())] = False
    assert counts.tolist() == [int((d[others] <= limit).sum()), 4, 1, int((d[others] > limit).sum())] and counts.sum() == 40
    assert status[np.flatnonzero(d == limit)[0]] == 0                       # closed: the tie is kept
    assert np.isfinite(sums).all() and not terms[status != 0].any()
    # the upper triangle is J J^T and the right-hand side J r: rebuild them from one used row
    i = int(np.flatnonzero(status == 0)[0])
    a, b, c = v[f[tri[i]]]
    N = np.cross(b - a, c - a)
    N /= np.linalg.norm(N)
    J = np.concatenate([np.cross(P[i], N), N, [P[i] @ N]])
    r = N @ (Y[i] - P[i])
    want = np.concatenate([np.outer(J, J)[np.triu_indices(7)], J * r, [r * r, d[i] ** 2]])
    assert np.allclose(terms[i], want, rtol=1e-13, atol=1e-18)
    with pytest.raises(ValueError, match='max_dist'):
        ma.host_sums(P, Y, tri, v, f, -1.0)


def test_evaluate_mesh_without_align_is_what_it_was():
    """align=None: the same keys and the same values as the call without the argument, from an equal rng state; and the rng ends
    in the same state.  With align set, the registration draws from a copy: the evaluation's own samples are the same."""
    v, f = ac.deformed_icosphere(1)
    v2, f2 = ac.deformed_icosphere(2)
    assert inspect.signature(mesheval.evaluate_mesh).parameters['align'].default is None
    assert inspect.signature(metrics.evaluate_mesh).parameters['align'].default is None
    rngs = [np.random.RandomState(7) for _ in range(3)]
    before = mesheval.evaluate_mesh((v, f), (v2, f2), num_samples=200, iou_points=300, rng=rngs[0])
    after = metrics.evaluate_mesh((v, f), (v2, f2), num_samples=200, iou_points=300, rng=rngs[1], align=None)
    assert list(before.keys()) == list(after.keys()) and 'alignment' not in after
    for k in before:
        if k == 'raw':
            assert list(before[k].keys()) == list(after[k].keys())
            assert all(np.array_equal(before[k][j], after[k][j]) for j in before[k])
        else:
            assert json.dumps(before[k], sort_keys=True) == json.dumps(after[k], sort_keys=True), k
    assert rngs[0].random_sample() == rngs[1].random_sample()
    aligned = mesheval.evaluate_mesh((v2, f2), (v2, f2), num_samples=200, iou_points=0, rng=rngs[2], align='rigid', align_options={'samples': 300})
    assert aligned['alignment']['converged'] and 'history' not in aligned['alignment'] and aligned['alignment']['mode'] == 'rigid'
    with pytest.raises(ValueError, match='align'):
        mesheval.evaluate_mesh((v, f), (v2, f2), num_samples=10, iou_points=0, align='affine')


def test_evaluate_mesh_with_align_undoes_a_known_similarity():
    """The host twin of the GPU test that shows what the feature is for (smaller, since the host query is quadratic): the prediction is
    the ground truth with a dent, so that their Chamfer distance is not zero; moved by a known similarity, align=None reports the
    misalignment, align='similarity' the distance of the unmoved pair.  The dent is one vertex fan (under 3 % of the area), which keep
    = 0.9 trims, so the true transform stays an exact fixed point; the gate 1e-9 relative is the issue's."""
    v, f, diag = target()
    dented = np.array(v)
    dented[0] *= 0.8
    K = ac.known(ac.STARTS[1], diag)
    kw = dict(num_samples=300, iou_points=0)
    base = mesheval.evaluate_mesh((dented, f), (v, f), rng=np.random.RandomState(5), **kw)
    off = mesheval.evaluate_mesh((ac.move(K, dented), f), (v, f), rng=np.random.RandomState(5), **kw)
    got = mesheval.evaluate_mesh((ac.move(K, dented), f), (v, f), rng=np.random.RandomState(5), align='similarity', align_options={'samples': 400}, **kw)
    print('chamfer: unmoved %.6e, moved %.6e, moved and aligned %.6e (relative difference %.3e)'
          % (base['chamfer'], off['chamfer'], got['chamfer'], abs(got['chamfer'] / base['chamfer'] - 1.0)))
    assert base['chamfer'] > 1e-5 * diag and off['chamfer'] > 5.0 * base['chamfer']
    assert abs(got['chamfer'] - base['chamfer']) <= 1e-9 * base['chamfer']
    assert all(e <= g for e, g in zip(ac.errors(got['alignment']['matrix'], K, diag), GATES))


def test_the_command_line_tool_on_the_host(tmp_path):
    from tools import align_mesh as tool
    v, f = ac.deformed_icosphere(1)
    diag = ac.diagonal(v)
    K = ac.known(ac.STARTS[0], diag)
    src, tgt, out, report = (str(tmp_path / n) for n in ('src.obj', 'tgt.obj', 'aligned.obj', 'm.json'))
    Mesh(ac.move(K, v), f).export(src)
    Mesh(v, f).export(tgt)
    r = tool.main([src, tgt, '--mode', 'similarity', '--samples', '200', '--seed', '1', '--device', 'cpu', '--out', out, '--matrix', report])
    assert all(e <= g for e, g in zip(ac.errors(r['matrix'], K, diag), GATES))
    moved = load_mesh(out)
    assert np.array_equal(moved.faces, f) and np.abs(moved.vertices - v).max() <= 1e-14
    with open(report) as fh:
        saved = json.load(fh)
    assert np.array_equal(np.asarray(saved['matrix']), r['matrix']) and saved['converged'] is True and os.path.getsize(report) > 0
    again = tool.main([src, tgt, '--mode', 'similarity', '--samples', '200', '--seed', '1', '--device', 'cpu', '--init', report])
    assert again['iterations'] <= 2
