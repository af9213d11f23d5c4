"""The stage-1 ray pipeline, kernel path by kernel path: psn_composite_fwd / _bwd (csrc/composite.hip) against the oracle's
formulas in float64, psn_first_crossing and psn_sample_points / _flagged (csrc/sample.hip) bit for bit against the torch
formulations of the reference -- on the cases of tests/ray_cases.py, whose coverage tests/test_ray_cpu.py asserts without a GPU.

Composite.  Every row of the dispatcher's table (six forward kernels, vector and non-vector row access, E = 1 .. 16, backward
E = 1 .. 16) at N = 1, 5, 37, 130 rays; every forward case with a black and a white background, every backward case in four
forms (white, black, d_acc = None, rgb = None).  Per kernel three ray counts around its grid cap C (C + 1, C + 5, 2 C + 3: the
second and third pass of the double-buffered grid-stride loops, the last pass in either register set, a last wave with one live
ray): flat 16385 / 16389 / 32771 x 96, opacity-only 131073 / 131077 / 262147 x 128 and x 64, several rays per wave 32769 / 32773 /
65539 x 64 and x 96, blocked 16385 / 16389 / 32771 x 130, backward 16385 / 16389 / 32771 x 96.  Offset inputs: alpha alone and rgb
alone as contiguous views that start one float into their buffer (4 mod 16), which takes the non-vector blocked kernel in place
of the vector, the several-rays and the four-rays-per-wave ones; the weights output is allocated by hip.composite_fwd and cannot
be offset through it.

Bound: helpers.assert_vs_truth, rtol 1e-5, atol ATOL_UNIT for w / rgb / acc and 'max' for the gradients (x SCALE of ray_cases for
S >= 512, measured to be 1): the kernel may have as many elements beyond the bound as the float32 CPU reference has beyond half of
it and a worst element of max(1, 2 x the reference's worst).  test_ray_cpu.py caps that reference (finite, <= 2 % beyond half
the bound, worst <= 4 x) and shows that seven wrong formulations fail this very check.
"""
import numpy as np
import pytest
import torch

from tests import ray_cases as rc
from tests.helpers import assert_vs_truth

pytestmark = pytest.mark.gpu
_WORST = {}   # (kernel, tensor) -> (worst r_hip, r_ref of that case, case)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _WORST:
        print('\n==== composite kernels vs float64: worst r_hip (the reference arithmetic in the same case), in units of the bound ====')
        for (kernel, name), (rh, rr, where) in sorted(_WORST.items()):
            print('%-22s %-10s r_hip %7.3f  r_ref %7.3f  (%s)' % (kernel, name, rh, rr, where))


def path_name(c):
    kernel, E, vec = rc.case_path(c)
    return '%s E=%d%s' % (kernel, E, ' vec' if vec and kernel == 'blocked' else '')


def check(c, name, got, truth, ref, atol, key=None):
    assert got.shape == truth.shape, '%s %s: shape %s vs %s' % (rc.case_id(c), name, tuple(got.shape), truth.shape)
    rtol, atol = rc.bound(c, atol)
    rh, rr = assert_vs_truth('%s %s' % (rc.case_id(c), name), got.cpu().numpy(), ref, truth, rtol, atol)
    print('%s %-16s r_hip %.3f r_ref %.3f' % (rc.case_id(c), name, rh, rr))
    k = (path_name(c), key or name)
    if rh > _WORST.get(k, (-1.0,))[0]:
        _WORST[k] = (rh, rr, rc.case_id(c))


def on_device(c, cuda):
    """The case's inputs on the device; the tensor named by c['mis'] as a view one float into its buffer."""
    inp = rc.make_inputs(c)
    d = {k: (None if v is None else v.to(cuda)) for k, v in inp.items()}
    if c['mis'] is not None:
        k = {'alpha': 'alpha', 'rgb': 'rgb'}[c['mis']]
        d[k] = rc.offset_by_one(inp[k], cuda)
        assert torch.equal(d[k].cpu(), inp[k])
    for k in ('alpha', 'rgb'):
        if d[k] is not None and c['mis'] != k:
            assert d[k].data_ptr() % 16 == 0
    return d


@pytest.mark.parametrize('c', rc.ALL_FWD, ids=rc.case_id)
def test_composite_forward_vs_float64(cuda, c):
    from psnerf_amd import hip
    d = on_device(c, cuda)
    ref = rc.reference(c)
    t, r = ref[torch.float64], ref[torch.float32]
    N, S, mode = c['N'], c['S'], c['mode']
    for white in (False, True):
        w, out, acc = hip.composite_fwd(d['alpha'], d['rgb'], white, need_weights=mode == 'w')
        bg = 'white' if white else 'black'
        if mode == 'w':
            check(c, 'w (%s)' % bg, w, t['w'], r['w'], rc.ATOL_UNIT, key='w')
        else:
            assert w is None
        check(c, 'acc (%s)' % bg, acc, t['acc'], r['acc'], rc.ATOL_UNIT, key='acc')
        if mode == 'op':
            assert out is None
        else:
            check(c, 'rgb_' + bg, out, t['rgb_' + bg], r['rgb_' + bg], rc.ATOL_UNIT)


@pytest.mark.parametrize('c', rc.ALL_BWD, ids=rc.case_id)
def test_composite_backward_vs_float64(cuda, c):
    from psnerf_amd import hip
    d = on_device(c, cuda)
    ref = rc.reference(c)
    t, r = ref[torch.float64], ref[torch.float32]
    for form in rc.BWD_FORMS:
        if form == 'no_rgb':
            da, dc = hip.composite_bwd(d['alpha'], None, None, d['c2'], True)
            assert dc is None
        else:
            da, dc = hip.composite_bwd(d['alpha'], d['rgb'], d['c1'], None if form == 'no_d_acc' else d['c2'], form != 'black')
            check(c, 'd_rgb ' + form, dc, t[form]['d_rgb'], r[form]['d_rgb'], 'max')
        check(c, 'd_alpha ' + form, da, t[form]['d_alpha'], r[form]['d_alpha'], 'max')


# one case per (mode, kernel, E, vector, offset): the N = 37 cases
KNOWN = list({(c['mode'],) + rc.case_path(c) + (c['mis'],): c for c in rc.FWD_CASES + rc.FWD_MIS_CASES if c['N'] == rc.MIS_N}.values())


@pytest.mark.parametrize('c', KNOWN, ids=rc.case_id)
def test_composite_known_answers_on_every_path(cuda, c):
    """All-zero opacities: acc == 0 and, under a white background, rgb == 1 exactly.  All-one opacities: w[:, 0] == 1 exactly and
    w[:, 1:] <= 2e-6 (w_1 = eps = 1e-6, the rest eps^2 and below); without a weights output the same statement on their sum,
    1 <= acc <= 1 + 2e-6."""
    from psnerf_amd import hip
    d = on_device(c, cuda)
    need_w = c['mode'] == 'w'
    place = (lambda x: rc.offset_by_one(x.cpu(), cuda)) if c['mis'] == 'alpha' else (lambda x: x)
    w, out, acc = hip.composite_fwd(place(torch.zeros_like(d['alpha'])), d['rgb'], True, need_weights=need_w)
    assert float(acc.abs().max()) == 0
    if need_w:
        assert float(w.abs().max()) == 0
    if d['rgb'] is not None:
        assert float((out - 1).abs().max()) == 0
    w, out, acc = hip.composite_fwd(place(torch.ones_like(d['alpha'])), d['rgb'], False, need_weights=need_w)
    if need_w:
        assert float((w[:, 0] - 1).abs().max()) == 0 and (c['S'] == 1 or float(w[:, 1:].abs().max()) < 2e-6)
    assert float(acc.min()) >= 1 and float(acc.max()) <= 1 + 2e-6
    if d['rgb'] is not None:   # the first sample's colour, and at most 2e-6 of the others
        assert float((out - d['rgb'][:, 0]).abs().max()) <= 2e-6


# ----------------------------------------------------------------------------------------------------------- first crossing
@pytest.mark.parametrize('M,N', rc.FC_CASES)
def test_first_crossing_on_constructed_profiles(cuda, M, N):
    """Bit for bit against the tensor formulation evaluated on the CPU: both flag bits on every ray, the four bracket rows where
    the mask bit is set, (0, 1, -1, 1) elsewhere."""
    from psnerf_amd import hip
    c = rc.crossing_case(M, N)
    val = c['occ'] - rc.FC_TAU
    mask, first_free, rows = rc.first_crossing_reference(val, c['u'], c['omu'], rc.FC_NEAR, c['far'])
    bracket, flags = hip.first_crossing(c['occ'].to(cuda), c['far'].to(cuda), c['u'].to(cuda), c['omu'].to(cuda), rc.FC_NEAR, rc.FC_TAU)
    bracket, flags = bracket.cpu(), flags.cpu()
    assert bracket.shape == (4, N) and flags.shape == (N,)
    bad = lambda sel: [c['names'][i] for i in sel.nonzero().reshape(-1).tolist()]
    assert torch.equal((flags & 1).bool(), mask), bad((flags & 1).bool() != mask)
    assert torch.equal((flags & 2).bool(), first_free), bad((flags & 2).bool() != first_free)
    assert not bool((flags & ~3).any())
    for row, (ref, benign) in enumerate(zip(rows, (0.0, 1.0, -1.0, 1.0))):
        want = torch.where(mask, ref, torch.full_like(ref, benign))
        assert torch.equal(bracket[row], want), 'bracket row %d: %s' % (row, bad(bracket[row] != want))


# ------------------------------------------------------------------------------------------------------------ sample points
@pytest.mark.parametrize('c0,c1,N,noise', rc.SP_CASES)
def test_sample_points_flagged_and_indexed(cuda, c0, c1, N, noise):
    """Mixed, all-hit and all-miss flags: the flagged launch == the two indexed launches == the CPU formulation, bit for bit;
    the depths of the first rays force the reference's sort to reorder (asserted on the CPU in test_ray_cpu.py)."""
    from psnerf_amd import hip
    case = rc.sample_case(c0, c1, N, noise)
    S = case['S']
    dev = {k: case[k].to(cuda) for k in ('cam', 'rays', 'far', 'dist')}
    nz = None if case['noise'] is None else case['noise'].to(cuda)
    u0, u1, um = rc.lin(c0, cuda), (rc.lin(c1, cuda) if c1 else None), rc.lin(S, cuda)
    for tag, flags in case['flags'].items():
        ref = rc.sample_reference(case, c0, c1, flags)
        fl = flags.to(cuda)
        out_f = torch.full((N, S, 3), float('nan'), device=cuda)
        hip.sample_points_flagged(dev['cam'], dev['rays'], dev['dist'], dev['far'], fl, out_f, rc.SP_NEAR, rc.SP_DELTA, u0, u1, um, noise=nz)
        out_i = torch.full((N, S, 3), float('nan'), device=cuda)
        hit_idx, miss_idx = fl.nonzero(as_tuple=True)[0], (~fl).nonzero(as_tuple=True)[0]
        if miss_idx.numel():
            hip.sample_points(dev['cam'], dev['rays'], dev['far'], out_i, False, rc.SP_NEAR, um, idx=miss_idx,
                              noise=None if nz is None else nz[miss_idx].contiguous())
        if hit_idx.numel():
            hip.sample_points(dev['cam'], dev['rays'], dev['far'], out_i, True, rc.SP_NEAR, u0, idx=hit_idx, dist=dev['dist'],
                              delta=rc.SP_DELTA, u1=u1, noise=None if nz is None else nz[hit_idx].contiguous())
        for name, out in (('flagged', out_f), ('indexed', out_i)):
            out = out.cpu()
            assert torch.equal(out, ref), '%s, %s flags: %d of %d rays differ, max |diff| = %g' % (
                name, tag, int((out != ref).any(-1).any(-1).sum()), N, float((out - ref).abs().max()))
