"""tests/loss_cases.py on the CPU: every definition, evaluated in float32, equals the oracle module it restates (loss terms to 1e-6
relative; the Adam definitions against torch.optim.Adam(foreach=True) / torch.optim.SparseAdam), and every case of the tables meets
the conditions under which float64 is a fair judge: gaps of the L1 pairs, |g| and |n - n_neighbour| of the surface normals, at most
3 % of the elements at a kink, and the float32 definition inside the plain bound on every tensor (r_ref <= 1).  Each test prints the
figures it asserts (pytest -s): the kink share and r_ref in units of the bound, per case."""
import numpy as np
import pytest
import torch

from oracle import stage1 as o1
from oracle import stage2 as o2
from tests import loss_cases as lc

REL = 1e-6


def close(a, b, what):
    a, b = float(a), float(b)
    assert abs(a - b) <= REL * abs(b), '%s: %r vs %r' % (what, a, b)


def report(family, cid, kinks, n, ratios, extra=''):
    share = kinks / max(n, 1)
    worst = max(ratios.values()) if ratios else 0.0
    print('%-8s %-22s kinks %6d of %9d (%.2f %%)  r_ref max %.4f  %s %s'
          % (family, cid, kinks, n, 100 * share, worst, ' '.join('%s %.3f' % kv for kv in sorted(ratios.items())), extra))
    assert share <= lc.KINK_CAP, '%s %s: %.2f %% of the elements at a kink' % (family, cid, 100 * share)
    for k, r in ratios.items():
        assert r <= 1.0, '%s %s %s: the float32 definition is at %.2f x the bound' % (family, cid, k, r)


def ref_ratios(r32, r64, skip=('terms', 'total')):
    return {k: lc.ratio(r32[k], r64[k]) for k in r64 if k not in skip}


# --------------------------------------------------------------------------- stage-2 losses
def _s2_oracle(case):
    """MainLoss + NormalLoss on the case's inputs -> (terms [6] with 0 for an absent term, total)."""
    t = lc.s2_inputs(case)
    w = lc.S2_WEIGHT
    out = {'network_object_mask': t['mask_a'][None], 'object_mask': t['mask_b'][None], 'sg_rgb_values': t['rgb']}
    inp = {}
    if t['alb'] is not None:
        out.update(albedo_values=t['alb'][None], albedo_jitter=t['alb_j'][None])
    if t['wgt'] is not None:
        out.update(rough_values=t['wgt'][None], rough_jitter=t['wgt_j'][None])
    if t['vis'] is not None:
        out.update(visibility=t['vis'], vis_train=t['vis'])
        inp.update(visibility=t['vis_gt'], light_vis_train=True, vis_train_gt=t['vis_gt'])
    main = o2.MainLoss(w[0], 'L2' if case['l2'] else 'L1', w[1], w[2], w[3])(out, {'rgb': t['rgb_gt']}, inp)
    terms = [main['sg_rgb_loss'], main['albedo_smooth_loss'], main['rough_smooth_loss'], main.get('vis_loss'), None, None]
    total = main['loss']
    if t['nrm'] is not None:
        out.update(normal_pred=t['nrm'][None], normal_values=t['nrm_gt'][None])
        if t['nrm_j'] is not None:
            out['normal_jitter'] = t['nrm_j'][None]
        nl = o2.NormalLoss(w[4], w[5])(out)
        terms[4], terms[5] = nl['normal_loss'], nl['normal_smooth_loss']
        total = total + nl['loss']
    return [0.0 if v is None else float(v) for v in terms], float(total)


@pytest.mark.parametrize('case', [c for c in lc.S2_CASES if c['count'] == 'host'], ids=lambda c: c['id'])
def test_stage2_definition_equals_oracle(case):
    """(the cases with a device count hand the same definition another divisor: the oracle has no such argument)"""
    t = lc.s2_inputs(case)
    inv, w, count_dev = lc.s2_scales(case)
    with torch.no_grad():
        terms, total = lc.stage2_loss(*lc.s2_args(t), t['mask_a'], t['mask_b'], case['l2'], inv, w, count_dev)
    o_terms, o_total = _s2_oracle(case)
    for i in range(6):
        close(terms[i], o_terms[i], 'term %d' % i)
    close(total, o_total, 'total')


@pytest.mark.parametrize('case', lc.S2_CASES, ids=lambda c: c['id'])
def test_stage2_case_conditions(case):
    t = lc.s2_inputs(case)
    for a, b in (('rgb', 'rgb_gt'), ('alb', 'alb_j'), ('wgt', 'wgt_j'), ('nrm', 'nrm_j')):
        if t[a] is not None and t[b] is not None and not (a == 'rgb' and case['l2']):
            assert lc.gap_ok(t[a], t[b]), a
    if t['vis'] is not None and not case['l2']:
        assert lc.gap_ok(t['vis'][..., 0], t['vis_gt']), 'vis'
    count = int(t['mask'].sum())
    assert (count == 0) == (case['masks'] == 'a_false')
    if case['masks'] == 'half' and case['N'] > 1:
        assert 0.3 * case['N'] <= count <= 0.7 * case['N']
    if case['poison']:
        assert all(bool(torch.isnan(t[k]).any()) for k in lc.S2_FLOATS) and 0 < count < case['N']
    r32, r64 = lc.s2_reference(case, torch.float32), lc.s2_reference(case, torch.float64)
    assert np.isfinite(r64['terms']).all() and all(np.isfinite(v).all() for v in r64.values())
    if count == 0 or case['count'] == 'dev0':
        assert all(not np.any(v) for v in r64.values()), 'an empty mask or a zero count: every term and gradient is 0'
    rel = float(np.max(np.abs(r32['terms'] - r64['terms']) / np.maximum(np.abs(r64['terms']), 1e-300)))
    assert rel <= lc.TERM_RTOL
    kinks, n = lc.s2_kinks(case)
    report('stage2', case['id'], kinks, n, ref_ratios(r32, r64), 'terms fp32 vs fp64 %.1e' % rel)


def test_stage2_count_forms_agree():
    """The host count and the same count on the device are one definition; twice the count halves every term and gradient."""
    by = {c['id']: c for c in lc.S2_CASES}
    host, dev, dev2 = (lc.s2_reference(by[k], torch.float64) for k in ('all-terms', 'count-dev', 'count-dev2'))
    assert sorted(host) == sorted(dev) == sorted(dev2)
    for k in host:
        assert np.allclose(dev[k], host[k], rtol=1e-12, atol=0) and np.allclose(2 * dev2[k], host[k], rtol=1e-12, atol=0), k


# --------------------------------------------------------------------------- stage-1 losses
@pytest.mark.parametrize('case', [c for c in lc.S1_CASES if c['route'] == 'finish' and c['n_rays'] == c['N'] and c['masks'] != 'empty'],
                         ids=lambda c: c['id'])
def test_stage1_definition_equals_oracle(case):
    """(not compared: scaled counts and n_rays != N, which oracle.stage1.Loss has no argument for, and the empty masks, where its
    BCE over no element is NaN and the kernels' max(count, 1) gives 0)"""
    t = lc.s1_inputs(case)
    with torch.no_grad():
        terms = lc.stage1_loss(*[t[k] for k in lc.S1_ARGS], case['n_rays'], case['weights'])
        one = lambda x: None if x is None else x[None]
        out = {'rgb': one(t['rgb']), 'diff_norm': None if t['diff'] is None else t['diff'][t['hit']], 'normal_pred': one(t['normal'])}
        ref = o1.Loss(*case['weights'])(out, one(t['rgb_gt']), one(t['normal_gt']), one(t['norm_mask']), one(t['acc']), one(t['mask_gt']),
                                         one(t['mask_valid']))
    for i, k in enumerate(('fullrgb_loss', 'grad_loss', 'normal_loss', 'mask_loss', 'loss')):
        close(terms[i], ref.get(k, 0.0), k)


@pytest.mark.parametrize('case', lc.S1_CASES, ids=lambda c: c['id'])
def test_stage1_case_conditions(case):
    t = lc.s1_inputs(case)
    assert lc.gap_ok(t['rgb'], t['rgb_gt']) and (t['normal'] is None or lc.gap_ok(t['normal'], t['normal_gt']))
    if t['acc'] is not None:
        a = t['acc'][18:] if case['acc'] == 'edges' else t['acc']
        inside = (a >= 0.02) & (a <= 0.98)
        outside = ((a <= -0.01) & (a >= -0.1001)) | ((a >= 1.01) & (a <= 1.1001))
        assert bool((inside | outside).all()) and (case['N'] < 255 or (bool(inside.any()) and bool(outside.any())))
        if case['acc'] == 'edges':
            got = {(float(x), float(y)) for x, y, v in zip(t['acc'][:18], t['mask_gt'][:18], t['mask_valid'][:18]) if v}
            assert got == {(float(np.float32(x)), float(np.float32(y))) for x in lc.S1_ACC_EDGES for y in lc.S1_GT_EDGES}
    r32, r64 = lc.s1_reference(case, torch.float32), lc.s1_reference(case, torch.float64)
    assert all(np.isfinite(v).all() for v in r64.values())
    if case['masks'] == 'empty':
        assert not r64['terms'][1:4].any() and not any(r64['d_' + k].any() for k in ('diff', 'normal', 'acc'))
    rel = float(np.max(np.abs(r32['terms'] - r64['terms']) / np.maximum(np.abs(r64['terms']), 1e-300)))
    assert rel <= lc.TERM_RTOL
    kinks, n = lc.s1_kinks(case)
    report('stage1', case['id'], kinks, n, ref_ratios(r32, r64), 'terms fp32 vs fp64 %.1e' % rel)


# --------------------------------------------------------------------------- surface normals
@pytest.mark.parametrize('spec', lc.SN_CASES, ids=lc.sn_id)
def test_surface_normals_definition_and_conditions(spec):
    t = lc.sn_inputs(spec)
    g, hit, N = t['g'], t['hit'], spec[0]
    with torch.no_grad():
        pred, diff = lc.surface_normals(g, hit)
        # oracle.stage1.Renderer, the three lines of its training forward on g [2 N, 1, 3]
        g3 = g[:, None, :]
        nrm = g3[:, 0, :] / (g3[:, 0, :].norm(2, dim=1).unsqueeze(-1) + 10 ** (-5))
        assert torch.equal(diff, torch.norm(nrm[:N] - nrm[N:], dim=-1))
        assert torch.equal(pred[hit], nrm[:N][hit]) and not pred[~hit].any()
        d64 = lc.surface_normals(g.double(), hit)[1]
    s = g.double().norm(dim=-1)
    assert bool(((s == 0) == t['zero']).all()) and bool((s[~t['zero']] >= lc.SN_MIN_G).all())
    assert bool(((d64 == 0) == t['same']).all()) and bool((d64[~t['same']] >= lc.SN_MIN_DIFF).all())
    assert {'mixed': 0 < int(hit.sum()) < N or N == 1, 'all': bool(hit.all()), 'none': not hit.any()}[spec[1]]
    r32, r64 = lc.sn_reference(spec, torch.float32), lc.sn_reference(spec, torch.float64)
    if N >= 255:
        assert not r64['diff_norm'][5] and (spec[2] != 'diff' or not r64['dg'][[5, N + 5]].any())   # the identical pair
    report('normals', lc.sn_id(spec), 3 * (int(t['zero'].sum()) + 2 * int(t['same'].sum())), g.numel(), ref_ratios(r32, r64, skip=()))


# --------------------------------------------------------------------------- Adam
def test_adam_definition_equals_torch_adam():
    """adam_update + adam_scalars in float32 = torch.optim.Adam(foreach=True) on the CPU, three steps, a learning rate per group."""
    g = torch.Generator().manual_seed(0)
    shapes, lrs = [(5,), (33, 7), (1025,)], [1e-3, 2e-3, 5e-4]
    params = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    opt = torch.optim.Adam([{'params': [p], 'lr': lr} for p, lr in zip(params, lrs)], betas=(lc.BETA1, lc.BETA2), eps=lc.ADAM_EPS, foreach=True)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    for step in range(1, 4):
        grads = [torch.randn(*s, generator=g) * 10.0 ** float(torch.randint(-6, 3, (1,), generator=g)) for s in shapes]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt.step()
        mine = [lc.adam_update(p, gr, m, v, lc.BETA1, lc.BETA2, lc.ADAM_EPS, *lc.adam_scalars(lr, step)) for (p, m, v), gr, lr in zip(mine, grads, lrs)]
        for (p, m, v), q in zip(mine, params):
            st = opt.state[q]
            for a, b, what in ((p, q.detach(), 'p'), (m, st['exp_avg'], 'm'), (v, st['exp_avg_sq'], 'v')):
                assert float((a - b).abs().max()) <= REL * float(b.abs().max()) and bool(((a - b).abs() <= 4 * REL * b.abs() + 1e-30).all()), (step, what)


def test_row_adam_definition_equals_torch_sparse_adam():
    """row_adam_update + row_adam_step_size in float32 = torch.optim.SparseAdam on the CPU: duplicate rows, changing row sets."""
    g = torch.Generator().manual_seed(1)
    n, lrs = 50, [5e-3, 1e-2]
    embs = [torch.nn.Embedding(n, c, sparse=True) for c in (3, 1)]
    opt = torch.optim.SparseAdam([{'params': list(e.parameters()), 'lr': lr} for e, lr in zip(embs, lrs)], betas=(lc.BETA1, lc.BETA2), eps=lc.ADAM_EPS)
    mine = [(e.weight.detach().clone(), torch.zeros(n, c), torch.zeros(n, c)) for e, c in zip(embs, (3, 1))]
    for step in range(1, 4):
        rows = torch.randint(0, n, (9,), generator=g)
        cs = [torch.randn(9, c, generator=g) for c in (3, 1)]
        opt.zero_grad()
        sum((e(rows) * c).sum() for e, c in zip(embs, cs)).backward()
        dense = [e.weight.grad.to_dense().clone() for e in embs]
        opt.step()
        mine = [lc.row_adam_update(p, gr, m, v, rows, lc.BETA1, lc.BETA2, lc.ADAM_EPS, lc.row_adam_step_size(lr, step))
                for (p, m, v), gr, lr in zip(mine, dense, lrs)]
        for (p, m, v), e in zip(mine, embs):
            st = opt.state[e.weight]
            for a, b, what in ((p, e.weight.detach(), 'p'), (m, st['exp_avg'], 'm'), (v, st['exp_avg_sq'], 'v')):
                assert float((a - b).abs().max()) <= REL * float(b.abs().max()), (step, what)


@pytest.mark.parametrize('name', sorted(lc.ADAM_CASES))
def test_adam_case_conditions(name):
    case = lc.adam_case(name)
    lengths, aligns = {n for n, _ in lc.ADAM_CASES[name]}, {a for _, a in lc.ADAM_CASES[name]}
    if name.startswith('seg'):
        assert lengths == set(lc.ADAM_LENGTHS) and aligns == set(lc.ADAM_ALIGN)
        assert name != 'seg33-3launches' or set(lc.ADAM_CASES[name]) == {(n, a) for n in lc.ADAM_LENGTHS for a in lc.ADAM_ALIGN}
    ends = 0
    for (off, goff, n), (_, (a, ga)) in zip(case['segs'], lc.ADAM_CASES[name]):
        assert off % 4 == a and goff % 4 == ga and off > ends   # a gap before every segment: the neighbours of a tail are outside
        ends = off + n
    mags = torch.cat([gr[goff:goff + n].abs() for gr in case['grads'] for _, goff, n in case['segs']])
    mags = mags[mags > 0]
    assert float(mags.min()) < 1e-7 and float(mags.max()) > 1e2 and bool(case['still'].any()) and not case['inside'].all()
    r32, r64 = lc.adam_reference(name, torch.float32), lc.adam_reference(name, torch.float64)
    still, out = case['still'].numpy(), ~case['inside'].numpy()
    assert np.array_equal(r64['p'][still], case['p'].double().numpy()[still]) and not r64['m'][still].any() and not r64['v'][still].any()
    assert all(np.array_equal(r64[k][out], case[k].double().numpy()[out]) for k in 'pmv')
    report('adam', name, 0, int(case['inside'].sum()), ref_ratios(r32, r64, skip=()))


@pytest.mark.parametrize('name', sorted(lc.ROW_ADAM_CASES))
def test_row_adam_case_conditions(name):
    case = lc.row_adam_case(name)
    shapes, n_idx, hi = lc.ROW_ADAM_CASES[name]
    for idx, _, _ in case['steps']:
        assert idx.numel() == n_idx and (n_idx < 2 or idx.unique().numel() < n_idx)   # duplicates
    (t32, touched), (t64, _) = lc.row_adam_reference(name, torch.float32), lc.row_adam_reference(name, torch.float64)
    ratios = {}
    for i, (tab, a, b, tch) in enumerate(zip(case['tables'], t32, t64, touched)):
        assert n_idx == 0 or tch.any()
        assert hi == 1 or not tch.all()
        for k, x, y, z in zip('pmv', a, b, tab):
            assert np.array_equal(y[~tch.numpy()], z.double().numpy()[~tch.numpy()])
            ratios['%s%d' % (k, i)] = lc.ratio(x, y)
    report('row_adam', name, 0, sum(r * c for r, c in shapes), ratios)
