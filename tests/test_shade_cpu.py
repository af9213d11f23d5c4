"""The cases and the float64 definition of tests/shade_cases.py, checked without a GPU: the reference reproduces the pinned
goldens it is built from, every case that tests/test_shade_gpu.py runs masks few of its pairs and sits on both sides of every
clamp, and the float32 reference arithmetic is measured against float64 under the GPU test's own bound (printed per tensor)."""
import os

import numpy as np
import pytest
import torch

from tests import shade_cases as sc
from tests.helpers import GOLDEN, assert_close, truth_ratios

ALL_CASES = sc.SG_CASES + sc.MF_CASES + sc.SG_RGB_LIGHT_CASES
MAX_AMBIGUOUS, MIN_SIDE, MIN_PAIRS = 0.10, 0.01, 300


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_reference_reproduces_the_pinned_goldens():
    """shade_cases.sg_brdf / mf_brdf in float64 against tests/golden/stage2_brdf.npz (the reference's own fp32 outputs; same gates
    as tests/test_oracle_golden.py::test_stage2_brdf), so this file cannot drift from the reference formulas."""
    g = np.load(os.path.join(GOLDEN, 'stage2_brdf.npz'), allow_pickle=False)
    d = lambda k: T(g[k]).double()
    lobe = torch.tensor([np.exp(i) for i in range(2, 11)], dtype=torch.float32).double()
    b, s = sc.sg_brdf(d('l'), d('v'), d('n'), d('albedo'), d('weights'), lobe, True)
    assert b.dtype == torch.float64
    assert_close(b, g['brdf'], 1e-6, 'brdf')
    assert_close(s, g['spec'], 1e-6, 'spec')
    mf = sc.mf_brdf(d('l2'), d('v'), d('n'), d('albedo'), d('rough'))
    assert mf.dtype == torch.float64
    assert_close(mf, g['mf'], 1e-5, 'microfacet')


def test_reference_forward_is_the_render_line():
    """One light-major case by hand: rows (l, n) -> l * Ns + n, cos on the raw inputs, visibility clamped, colour clamped; and the
    raw specular sum of ambiguous_pairs() is what SGBasis clamps."""
    spec = sc.SG_CASES[6]
    c, r = sc.make_case(spec), sc.reference(spec, torch.float64)
    L, Ns = c['L'], c['Ns']
    assert r['rgb'].shape == (L * Ns, 3) and r['spec'].shape == (L * Ns, 3) and r['d_vis'].shape == (L * Ns, 1)
    assert np.array_equal(r['spec'], np.maximum(c['info']['raw'], 0.0))
    l, n = 3, 17
    row = l * Ns + n
    cos = float(c['light_dir'][l].double() @ c['normal'][n].double())
    pre = (c['albedo'][n].double().numpy() + r['spec'][row]) * float(c['light_int'][l, 0]) * cos * float(c['vis_in'][row, 0].clamp(0, 1))
    assert np.allclose(r['pre'][row], pre, rtol=1e-13, atol=0) and np.array_equal(r['rgb'][row], np.clip(r['pre'][row], 0, 1))


@pytest.mark.parametrize('spec', ALL_CASES, ids=sc.case_id)
def test_case_conditions(spec):
    """Conditions on the float64 reference alone: at most 10 % of the pairs are ambiguous (a test must not hide a failure by
    masking its inputs), the upstream gradients vanish exactly there, and a case of >= 300 pairs has at least 1 % of its
    non-ambiguous pairs on each side of each mask."""
    c = sc.make_case(spec)
    amb, sides = sc.coverage(spec)
    print('%s: %d pairs, ambiguous %.2f %%; ' % (sc.case_id(spec), c['L'] * c['Ns'], 100 * amb)
          + ', '.join('%s %.1f %%' % (k, 100 * v) for k, v in sides.items()))
    assert amb <= MAX_AMBIGUOUS
    a = c['ambiguous']
    assert a.shape == (c['L'] * c['Ns'],) and float(c['g_rgb'][a].abs().sum()) == 0 and bool((c['g_rgb'][~a] != 0).all())
    if c.get('g_spec_in') is not None:
        assert float(c['g_spec_in'][a].abs().sum()) == 0
    if c['vis_in'] is not None and c['L'] * c['Ns'] >= 60:
        assert bool((c['vis_in'] == 0).any()) and bool((c['vis_in'] == 1).any())
    if c['L'] * c['Ns'] >= MIN_PAIRS:
        for k, share in sides.items():
            assert MIN_SIDE <= share <= 1 - MIN_SIDE, '%s: %.2f %% of the non-ambiguous pairs' % (k, 100 * share)


def test_ambiguity_is_cancellation_not_smallness():
    """nb = 1: a back-facing half vector makes w D tiny, never cancelled; no such pair may be masked for its specular sum."""
    for spec in sc.SG_CASES:
        if spec['nb'] == 1:
            c = sc.make_case(spec)
            raw = c['info']['raw']
            assert (np.abs(raw) > 0).all()
            pre = c['info']['pre']
            colour = ((np.abs(pre) < sc.MARGIN_COLOUR) | (np.abs(pre - 1) < sc.MARGIN_COLOUR)).any(-1)
            assert not (c['ambiguous'].numpy() & ~colour).any()


@pytest.mark.parametrize('kernel', ['sg', 'mf'])
def test_reference_arithmetic_vs_float64(kernel):
    """Measurement: the float32 CPU evaluation of the same formulas against float64 under the GPU test's bound
    1e-5 |truth| + 1e-5 max|truth| -- what the allowance of the GPU test is derived from.  Printed, worst case per tensor."""
    worst = {}
    for spec in (sc.SG_CASES if kernel == 'sg' else sc.MF_CASES):
        t, r = sc.reference(spec, torch.float64), sc.reference(spec, torch.float32)
        keep = ~sc.make_case(spec)['ambiguous'].numpy()
        for k in sorted(t):
            if k == 'pre':
                continue
            a, b = (r[k], t[k]) if not (kernel == 'mf' and k == 'rgb') else (r[k][keep], t[k][keep])
            assert np.isfinite(a).all() and np.isfinite(b).all(), (sc.case_id(spec), k)
            if not np.abs(b).max() > 0:
                continue
            _, r_ref, _, _, _ = truth_ratios(a, a, b, 1e-5, 'max')
            if float(r_ref.max()) > worst.get(k, (-1, ''))[0]:
                worst[k] = (float(r_ref.max()), sc.case_id(spec))
    print('\n%s: float32 reference arithmetic vs float64, worst |error| / bound per tensor' % kernel)
    for k, (v, where) in sorted(worst.items()):
        print('  %-12s %6.3f  (%s)' % (k, v, where))
    assert set(worst) >= {'rgb', 'd_light_dir', 'd_light_int', 'd_normal', 'd_albedo', 'd_vis'}
