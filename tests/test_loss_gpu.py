"""The kernels that produce the training loss and apply the update, called directly and compared with the float64 definitions of
tests/loss_cases.py, launch path by launch path: hip.stage2_loss_fwd / bwd (csrc/loss.hip), hip.stage1_loss_fwd / terms / bwd and
hip.surface_normals_fwd / bwd (csrc/loss1.hip), hip.adam_flat (csrc/small.hip) and hip.row_adam (csrc/loss.hip); one pass each through
ops.Stage2Losses, ops.Stage1Losses and ops.SurfaceNormals under autograd for the gradient slots.  The case ids name the path: see the
tables in loss_cases.py.

Tolerance: none chosen.  Tensors (gradients, normals, parameters, moments): bound = 1e-5 |truth| + 1e-5 max|truth| per tensor, r_ref =
the float32 definition on the CPU against truth, r_hip = the kernel against truth, both in units of the bound; the kernel may have as
many elements beyond the bound as the definition has beyond half of it and a worst element of max(1, 2 max r_ref) (tests/helpers.py).
Scalar loss terms and the total: |kernel - truth| <= 2e-6 |truth|.  Exact (torch.equal / == 0): gradients at masked-out pixels, at ties
and under a zero count, d_vis[..., 1:], optimiser elements outside the segments / rows, every device-scalar form against its host form.

Measured on an MI355X (gfx950), worst case over all cases, in units of the bound: r_hip (r_ref of the same case).
Every tensor of every kernel stays inside 4 % of the plain bound; the allowance is not drawn on.
    stage2_loss      d_rgb 0.005 (0.005)   d_alb / d_alb_j 0.005 (0.001)   d_wgt / d_wgt_j 0.004 (0.001)   d_vis 0.005 (0.005)
                     d_nrm 0.010 (0.009)   d_nrm_j 0.004 (0.002)           six terms and the total: 2.1e-07 relative (N262444-L1)
    stage1_loss      d_rgb 0.003 (0.001)   d_diff 0.003 (0.003)   d_normal 0.002 (0.002)   d_acc 0.006 (0.006)
                     four terms and the total: 3.3e-07 relative (N16684)
    surface_normals  normal_pred 0.007 (0.007)   diff_norm 0.018 (0.015)   dg 0.038 (0.038)
    adam_flat        p 0.007 (0.007)   m 0.006 (0.006)   v 0.010 (0.010)
    row_adam         p 0.005 (0.005)   m 0.006 (0.006)   v 0.007 (0.007)
    ops.Stage2Losses / ops.Stage1Losses / ops.SurfaceNormals under autograd: the figures of their kernels in the same case
    (at most 0.005 / 0.003 / 0.017; terms 1.0e-07 / 1.1e-07 relative).
The gradients of the L1 terms are k sign(x - y) with k a product of three float32 factors, the optimiser updates a handful of
operations per element: both evaluations round a few times and land at a hundredth of the bound.  What these tests are for is not
that margin but the indexing around it -- a light, a pixel, a tail or a row that a launch path skips or visits twice is off by the
whole value.
"""
import numpy as np
import pytest
import torch

from tests import loss_cases as lc
from tests.helpers import assert_vs_truth

pytestmark = pytest.mark.gpu
_WORST = {}   # (kernel, tensor) -> (worst r_hip, r_ref of that case, case)
_TERMS = {}   # kernel -> (worst |kernel - truth| / |truth| of a scalar term, case)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _WORST:
        print('\n==== loss and optimiser kernels vs float64: worst r_hip (the float32 definition in the same case) ====')
        for (kernel, name), (rh, rr, where) in sorted(_WORST.items()):
            print('%-16s %-12s r_hip %7.3f  r_ref %7.3f  (%s)' % (kernel, name, rh, rr, where))
        for kernel, (rel, where) in sorted(_TERMS.items()):
            print('%-16s scalar terms: worst |kernel - truth| / |truth| %.2e  (%s)' % (kernel, rel, where))


def check(kernel, where, name, got, ref, truth):
    """One tensor of one case against truth under the measured allowance; records the worst figures per kernel and tensor."""
    got = got.detach().cpu().numpy()
    assert got.shape == truth.shape, '%s %s %s: shape %s vs %s' % (kernel, where, name, got.shape, truth.shape)
    rh, rr = assert_vs_truth('%s %s %s' % (kernel, where, name), got, ref, truth, lc.RTOL, 'max')
    print('%s %s %s: r_hip %.3f (r_ref %.3f)' % (kernel, where, name, rh, rr))
    if rh > _WORST.get((kernel, name), (-1.0,))[0]:
        _WORST[(kernel, name)] = (rh, rr, where)


def check_terms(kernel, where, got, truth):
    """Scalar terms: |kernel - truth| <= 2e-6 |truth| each (a truth of 0 is matched exactly)."""
    got, truth = got.detach().double().cpu().numpy().reshape(-1), np.asarray(truth, dtype=np.float64).reshape(-1)
    assert got.shape == truth.shape and np.isfinite(got).all(), (where, got)
    err = np.abs(got - truth)
    rel = float(np.max(err / np.maximum(np.abs(truth), 1e-300)))
    print('%s %s terms: worst relative error %.2e' % (kernel, where, rel))
    assert (err <= lc.TERM_RTOL * np.abs(truth)).all(), '%s %s: terms %r vs truth %r' % (kernel, where, got, truth)
    if rel > _TERMS.get(kernel, (-1.0,))[0]:
        _TERMS[kernel] = (rel, where)


def to_dev(t, cuda):
    return None if t is None else t.to(cuda)


# --------------------------------------------------------------------------- stage-2 losses
def s2_run(case, cuda):
    """-> (out [7] = six terms + total, {name: gradient}) of hip.stage2_loss_fwd / bwd on the case, called as ops.Stage2Losses calls them."""
    from psnerf_amd import hip
    t = lc.s2_inputs(case)
    inv, w, count = lc.s2_scales(case)
    count_dev = None if count is None else torch.tensor([count], dtype=torch.float32, device=cuda)
    d = {k: to_dev(t[k], cuda) for k in lc.S2_FLOATS}
    ma, mb = t['mask_a'].to(cuda), t['mask_b'].to(cuda)
    out = hip.stage2_loss_fwd(*[d[k] for k in lc.S2_FLOATS], ma, mb, case['l2'], inv, w, count_dev)
    k = [wi * di for wi, di in zip(w, inv)]
    need = {n for n in ('rgb', 'alb', 'wgt', 'vis', 'nrm') if d[n] is not None}
    g = torch.tensor([lc.G_UP], dtype=torch.float32, device=cuda)
    grads = hip.stage2_loss_bwd(g, d['rgb'], d['rgb_gt'], k[0], d['alb'], d['alb_j'], k[1], d['wgt'], d['wgt_j'], k[2], d['vis'], d['vis_gt'], k[3],
                                d['nrm'], d['nrm_gt'], d['nrm_j'], k[4], k[5], ma, mb, case['l2'], need, count_dev)
    return out, grads


def s2_exact(case, grads):
    """What holds bit for bit: nothing is NaN; the masked-out pixels, the ties and channels 1, 2 of d_vis have gradient 0."""
    t = lc.s2_inputs(case)
    m, ties = t['mask'], t['ties']
    for name, gr in grads.items():
        gr = gr.cpu()
        assert bool(torch.isfinite(gr).all()), name
        off = gr[:, ~m] if name in ('rgb', 'vis') else gr[~m]
        assert not off.any(), '%s: a gradient at a masked-out pixel' % name
    for name, tie in (('rgb', ties['rgb']), ('alb', ties['alb']), ('alb_j', ties['alb']), ('wgt', ties['wgt']), ('wgt_j', ties['wgt'])):
        if name in grads:
            assert not grads[name].cpu()[tie].any(), '%s: a gradient at a tie' % name
    if 'vis' in grads:
        gv = grads['vis'].cpu()
        assert not gv[..., 1:].any() and not gv[..., 0][ties['vis']].any()
    if 'nrm_j' in grads:
        assert not grads['nrm_j'].cpu()[ties['nrm']].any()   # (d_nrm also carries the term against nrm_gt there)


@pytest.mark.parametrize('case', lc.S2_CASES, ids=lambda c: c['id'])
def test_stage2_loss_kernels(cuda, case):
    out, grads = s2_run(case, cuda)
    r32, r64 = lc.s2_reference(case, torch.float32), lc.s2_reference(case, torch.float64)
    check_terms('stage2_loss', case['id'], out, np.concatenate([r64['terms'], r64['total'].reshape(1)]))
    assert sorted('d_' + k for k in grads) == sorted(k for k in r64 if k.startswith('d_'))
    s2_exact(case, grads)
    for name, gr in sorted(grads.items()):
        check('stage2_loss', case['id'], 'd_' + name, gr, r32['d_' + name], r64['d_' + name])
    if case['count'] == 'dev0' or case['masks'] == 'a_false':
        assert not out.cpu().any() and not any(bool(gr.any()) for gr in grads.values())


def test_stage2_loss_count_forms(cuda):
    """The same count from the host (folded into inv_denom) and from the device give the same terms and gradients, each within its
    bound of the one truth; twice the count on the device halves them -- exactly: a division by 2 c."""
    by = {c['id']: c for c in lc.S2_CASES}
    (o_h, g_h), (o_d, g_d), (o_2, g_2) = (s2_run(by[k], cuda) for k in ('all-terms', 'count-dev', 'count-dev2'))
    truth, r32 = lc.s2_reference(by['all-terms'], torch.float64), lc.s2_reference(by['all-terms'], torch.float32)
    for out in (o_h, o_d, 2 * o_2):
        check_terms('stage2_loss', 'count forms', out, np.concatenate([truth['terms'], truth['total'].reshape(1)]))
    for name in g_h:
        for gr in (g_h[name], g_d[name], 2 * g_2[name]):
            check('stage2_loss', 'count forms', 'd_' + name, gr, r32['d_' + name], truth['d_' + name])
    assert torch.equal(2 * o_2, o_d) and all(torch.equal(2 * g_2[k], g_d[k]) for k in g_d)


def test_stage2_losses_autograd_slots(cuda):
    """ops.Stage2Losses: the gradients land on the tensors they belong to, and an input that asked for none gets none."""
    from psnerf_amd import ops
    case = next(c for c in lc.S2_CASES if c['id'] == 'L17')
    t = lc.s2_inputs(case)
    inv, w, _ = lc.s2_scales(case)
    r32, r64 = lc.s2_reference(case, torch.float32), lc.s2_reference(case, torch.float64)
    for wanted in (lc.S2_LEAVES, ('alb_j', 'vis'), ('rgb', 'nrm_j')):
        d = {k: t[k].to(cuda).requires_grad_(k in wanted) for k in lc.S2_FLOATS}
        total, terms = ops.Stage2Losses.apply(*[d[k] for k in lc.S2_FLOATS], t['mask_a'].to(cuda), t['mask_b'].to(cuda), case['l2'], inv, w, None)
        assert total.requires_grad and not terms.requires_grad
        check_terms('Stage2Losses', 'L17 ' + '+'.join(wanted), torch.cat([terms, total.detach().reshape(1)]), np.concatenate([r64['terms'], r64['total'].reshape(1)]))
        total.backward(torch.tensor(lc.G_UP, device=cuda))
        for k in lc.S2_FLOATS:
            if k in wanted:
                check('Stage2Losses', 'L17 ' + '+'.join(wanted), 'd_' + k, d[k].grad, r32['d_' + k], r64['d_' + k])
            else:
                assert d[k].grad is None, k
    # straight from the backward: None in the slot of everything that is no prediction
    d = {k: t[k].to(cuda).requires_grad_(k in lc.S2_LEAVES) for k in lc.S2_FLOATS}
    total, _ = ops.Stage2Losses.apply(*[d[k] for k in lc.S2_FLOATS], t['mask_a'].to(cuda), t['mask_b'].to(cuda), case['l2'], inv, w, None)
    slots = total.grad_fn.apply(torch.tensor(lc.G_UP, device=cuda), None)
    assert len(slots) == 17
    for i, k in enumerate(lc.S2_FLOATS):
        assert (slots[i] is not None) == (k in lc.S2_LEAVES), k
        if k in lc.S2_LEAVES:
            check('Stage2Losses', 'L17 slots', 'd_' + k, slots[i], r32['d_' + k], r64['d_' + k])
    assert all(s is None for s in slots[11:])


# --------------------------------------------------------------------------- stage-1 losses
def s1_run(case, cuda):
    """-> (sums [8], terms [5], {name: gradient}) of hip.stage1_loss_fwd (/ stage1_loss_terms) / stage1_loss_bwd."""
    from psnerf_amd import hip
    t = lc.s1_inputs(case)
    d = {k: to_dev(t[k], cuda) for k in lc.S1_ARGS}
    w = case['weights']
    sums, terms = hip.stage1_loss_fwd(*[d[k] for k in lc.S1_ARGS], case['n_rays'], w, finish=case['route'] == 'finish')
    local = sums.clone()
    if case['route'] == 'terms':
        assert terms is None
        sums[4:7] *= torch.tensor(lc.S1_COUNT_SCALE, device=cuda)   # what the all-reduce does under data parallelism
        terms = hip.stage1_loss_terms(sums, case['n_rays'], w, d['diff'] is not None and w[1] != 0.0, d['normal'] is not None, d['acc'] is not None)
    g = torch.tensor([lc.G_UP], dtype=torch.float32, device=cuda)
    grads = hip.stage1_loss_bwd(g, sums, d['rgb'], d['rgb_gt'], d['hit'], d['normal'], d['normal_gt'], d['norm_mask'], d['acc'], d['mask_gt'],
                                d['mask_valid'], case['n_rays'], w, lc.s1_need(case))
    return local, terms, grads


@pytest.mark.parametrize('case', lc.S1_CASES, ids=lambda c: c['id'])
def test_stage1_loss_kernels(cuda, case):
    t = lc.s1_inputs(case)
    sums, terms, grads = s1_run(case, cuda)
    r32, r64 = lc.s1_reference(case, torch.float32), lc.s1_reference(case, torch.float64)
    counts = [0.0 if t[k] is None else float(t[k].sum()) for k in ('hit', 'norm_mask', 'mask_valid')]
    assert sums[4:7].tolist() == counts, 'the hit / norm_mask / mask_valid counts in sums[4:7]'
    check_terms('stage1_loss', case['id'], terms, r64['terms'])
    assert sorted(grads) == sorted(lc.s1_need(case))
    for name, gr in sorted(grads.items()):
        assert bool(torch.isfinite(gr).all()), name
        check('stage1_loss', case['id'], 'd_' + name, gr, r32['d_' + name], r64['d_' + name])
    for name, mask in (('diff', 'hit'), ('normal', 'norm_mask'), ('acc', 'mask_valid')):
        if name in grads:
            assert not grads[name].cpu()[~t[mask]].any(), '%s: a gradient outside %s' % (name, mask)
    for name in ('rgb', 'normal'):
        if name in grads:
            assert not grads[name].cpu()[t['ties'][name]].any(), '%s: a gradient at a tie' % name
    if 'acc' in grads:
        assert not grads['acc'].cpu()[(t['acc'] < 0) | (t['acc'] > 1)].any(), 'acc outside [0, 1] passes no gradient'
    if case['masks'] == 'empty':
        assert not terms[1:4].cpu().any() and not any(bool(grads[k].any()) for k in ('diff', 'normal', 'acc'))


def test_stage1_losses_autograd_slots(cuda):
    """ops.Stage1Losses, plain and through the reduce_counts hook (the 'terms' route), under autograd."""
    from psnerf_amd import ops
    by = {c['id']: c for c in lc.S1_CASES}
    for cid, wanted in (('N257', lc.S1_LEAVES), ('N257', ('diff', 'acc')), ('terms-route-N257', lc.S1_LEAVES)):
        case = by[cid]
        t = lc.s1_inputs(case)
        r32, r64 = lc.s1_reference(case, torch.float32), lc.s1_reference(case, torch.float64)
        d = {k: t[k].to(cuda) for k in lc.S1_ARGS}
        for k in wanted:
            d[k].requires_grad_(True)
        scale = torch.tensor(lc.S1_COUNT_SCALE, device=cuda)
        hook = (lambda c: c.mul_(scale)) if case['route'] == 'terms' else None
        loss, terms = ops.Stage1Losses.apply(*[d[k] for k in lc.S1_ARGS], case['n_rays'], case['weights'], hook)
        assert not terms.requires_grad
        where = '%s %s' % (cid, '+'.join(wanted))
        check_terms('Stage1Losses', where, terms, r64['terms'])
        loss.backward(torch.tensor(lc.G_UP, device=cuda))
        for k in lc.S1_ARGS:
            if k in wanted:
                check('Stage1Losses', where, 'd_' + k, d[k].grad, r32['d_' + k], r64['d_' + k])
            else:
                assert d[k].grad is None, k
        if wanted == lc.S1_LEAVES and hook is None:
            d = {k: t[k].to(cuda).requires_grad_(k in wanted) for k in lc.S1_ARGS}
            loss, _ = ops.Stage1Losses.apply(*[d[k] for k in lc.S1_ARGS], case['n_rays'], case['weights'], None)
            slots = loss.grad_fn.apply(torch.tensor(lc.G_UP, device=cuda), None)
            assert len(slots) == 13 and [i for i, s in enumerate(slots) if s is not None] == [0, 2, 4, 7]


# --------------------------------------------------------------------------- surface normals
@pytest.mark.parametrize('spec', lc.SN_CASES, ids=lc.sn_id)
def test_surface_normals_kernels(cuda, spec):
    from psnerf_amd import hip
    t = lc.sn_inputs(spec)
    N, where = spec[0], lc.sn_id(spec)
    g, hit = t['g'].to(cuda), t['hit'].to(cuda)
    pred, diff = hip.surface_normals_fwd(g, hit)
    dg = hip.surface_normals_bwd(g, hit, t['d_norm_pred'].to(cuda) if spec[2] in ('both', 'norm_pred') else None,
                                 t['d_diff'].to(cuda) if spec[2] in ('both', 'diff') else None)
    r32, r64 = lc.sn_reference(spec, torch.float32), lc.sn_reference(spec, torch.float64)
    for name, got in (('normal_pred', pred), ('diff_norm', diff), ('dg', dg)):
        assert bool(torch.isfinite(got).all()), name
        check('surface_normals', where, name, got, r32[name], r64[name])
    assert not pred.cpu()[~t['hit']].any()
    assert not pred.cpu()[t['zero'][:N] & t['hit']].any(), 'n = 0 / (0 + eps) = 0'
    assert not diff.cpu()[t['same']].any(), 'identical g: diff_norm is exactly 0'
    if spec[2] == 'diff' and t['same'].any():
        assert not dg.cpu()[torch.cat([t['same'], t['same']])].any(), 'd |x| = 0 at x = 0'


def test_surface_normals_autograd_slots(cuda):
    from psnerf_amd import ops
    spec = lc.SN_CASES[2]
    t = lc.sn_inputs(spec)
    r32, r64 = lc.sn_reference(spec, torch.float32), lc.sn_reference(spec, torch.float64)
    g, hit = t['g'].to(cuda).requires_grad_(True), t['hit'].to(cuda)
    pred, diff = ops.SurfaceNormals.apply(g, hit)
    ((pred * t['d_norm_pred'].to(cuda)).sum() + (diff * t['d_diff'].to(cuda)).sum()).backward()
    assert hit.grad is None
    check('SurfaceNormals', lc.sn_id(spec), 'dg', g.grad, r32['dg'], r64['dg'])
    pred, diff = ops.SurfaceNormals.apply(g, hit)
    slots = pred.grad_fn.apply(t['d_norm_pred'].to(cuda), t['d_diff'].to(cuda))
    assert len(slots) == 2 and slots[1] is None and torch.equal(slots[0], g.grad)


# --------------------------------------------------------------------------- adam_flat
def adam_run(name, cuda, dev_scalars):
    from psnerf_amd import hip
    case = lc.adam_case(name)
    p, m, v = (case[k].to(cuda) for k in 'pmv')
    for gr, sc in zip(case['grads'], case['scalars']):
        segs = [(off, goff, n, ns, bc) for (off, goff, n), (ns, bc) in zip(case['segs'], sc)]
        scal = None
        if dev_scalars:
            scal = torch.tensor(sc, dtype=torch.float64).float().to(cuda)
            segs = [(off, goff, n, 0.0, 1.0) for off, goff, n, _, _ in segs]   # the host values must not be what is used
        hip.adam_flat(p, gr.to(cuda), m, v, segs, lc.BETA1, lc.BETA2, lc.ADAM_EPS, scalars_dev=scal)
    return {'p': p, 'm': m, 'v': v}


@pytest.mark.parametrize('name', sorted(lc.ADAM_CASES))
def test_adam_flat_kernel(cuda, name):
    case = lc.adam_case(name)
    host, dev = adam_run(name, cuda, False), adam_run(name, cuda, True)
    r32, r64 = lc.adam_reference(name, torch.float32), lc.adam_reference(name, torch.float64)
    outside, still = ~case['inside'], case['still']
    for k in 'pmv':
        got = host[k].cpu()
        assert torch.equal(got[outside], case[k][outside]), '%s: an element outside the segments changed' % k
        assert torch.equal(got[still], case[k][still]), '%s: g = m = v = 0 and the element moved' % k
        assert torch.equal(dev[k], host[k]), '%s: scalars_dev and host scalars differ' % k
        check('adam_flat', name, k, host[k], r32[k], r64[k])


# --------------------------------------------------------------------------- row_adam
def row_adam_run(name, cuda, dev_sizes):
    from psnerf_amd import hip
    case = lc.row_adam_case(name)
    tabs = [tuple(t.to(cuda) for t in tab) for tab in case['tables']]
    for idx, grads, sizes in case['steps']:
        items = [(p, gr.to(cuda), m, v, lc.BETA1, lc.BETA2, lc.ADAM_EPS, 0.0 if dev_sizes else ss) for (p, m, v), gr, ss in zip(tabs, grads, sizes)]
        hip.row_adam(items, idx.to(cuda), step_sizes_dev=torch.tensor(sizes, dtype=torch.float64).float().to(cuda) if dev_sizes else None)
    return tabs


@pytest.mark.parametrize('name', sorted(lc.ROW_ADAM_CASES))
def test_row_adam_kernel(cuda, name):
    case = lc.row_adam_case(name)
    host, dev = row_adam_run(name, cuda, False), row_adam_run(name, cuda, True)
    (t32, touched), (t64, _) = lc.row_adam_reference(name, torch.float32), lc.row_adam_reference(name, torch.float64)
    for i, (tab, h, d, a, b, tch) in enumerate(zip(case['tables'], host, dev, t32, t64, touched)):
        for k, x0, xh, xd, ref, truth in zip('pmv', tab, h, d, a, b):
            assert torch.equal(xh.cpu()[~tch], x0[~tch]), '%s of table %d: an untouched row changed' % (k, i)
            assert torch.equal(xd, xh), '%s of table %d: step_sizes_dev and host step sizes differ' % (k, i)
            check('row_adam', name, k, xh, ref, truth)
        if lc.ROW_ADAM_CASES[name][1] == 0:
            assert all(torch.equal(x.cpu(), x0) for x, x0 in zip(h, tab)), 'an empty index list changes nothing'
