"""The derivation behind psn_geo_point_grad, checked without any kernel in float64 torch:

    d loss / d p = J(p)^T (W_0^T dZ_0 + W_sk[:, d_a:]^T dZ_sk) + H(p)[g_pe, d_grad]

with dZ_l = the cotangent of the pre-activation of layer l under the WHOLE objective (value pass and gradient sweep), g_pe =
d logit / d pe and d_grad = d loss / d grad -- against pts.grad of tests/engine_cases.geo_field; and the numpy statement of the
kernel's contract (tests/geo_dp_cases.point_grad_contract, the truth of tests/test_geo_dp_gpu.py) against torch autograd."""
import numpy as np
import pytest
import torch

from tests import engine_cases as ec
from tests import geo_dp_cases as dc


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize('use', [ec._ALL, ('logit', 'feat'), ('grad',)], ids=lambda u: '+'.join(u))
def test_two_term_formula_equals_autograd_in_float64(use):
    spec = dict(Q=65, feat_rows=None, with_grad=True, use=use)
    case = ec.geo_case(spec)
    params, octaves, skips, scale = ec.geo_weights()
    P = [t.double() for t in params]
    pts = case['pts'].detach().double().requires_grad_(True)
    logit, feat, grad, pe, zs = dc.geo_field_parts(pts, P, octaves, skips, scale)
    ref = ec.geo_field(case['pts'].detach().double().requires_grad_(True), P, octaves, skips, scale)   # the restatement IS that function
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip((logit, feat, grad), ref))
    sk = skips[0]
    g_pe = torch.autograd.grad(logit.sum(), pe, retain_graph=True)[0]
    for z in (zs[0], zs[sk]):   # (after the call above: a retained gradient collects from every backward pass through the tensor)
        z.retain_grad()
    ec.geo_objective(case, logit, feat, grad).backward()
    d_pe = 3 + 6 * octaves
    d_a = P[2 * sk].shape[1] - d_pe
    second = 'grad' in use
    got = dc.point_grad_contract(pts, octaves, scale, zs[0].grad, P[0], dzs=zs[sk].grad, ws=P[2 * sk][:, d_a:],
                                 g_pe=g_pe if second else None, d_grad=case['c_grad'] if second else None)
    truth = pts.grad.numpy()
    assert np.abs(truth).max() > 0
    assert _rel(got, truth) <= 1e-10, _rel(got, truth)
    if second:   # the second term is no rounding matter: without it the formula is wrong
        first_only = dc.point_grad_contract(pts, octaves, scale, zs[0].grad, P[0], dzs=zs[sk].grad, ws=P[2 * sk][:, d_a:])
        assert _rel(first_only, truth) > 1e-6


def test_geo_reference_dp_extends_geo_reference():
    case = ec.geo_case(ec.GEO_CASES[1])
    a, b = dc.geo_reference_dp(case, torch.float64), ec.geo_reference(case, torch.float64)
    assert sorted(a) == sorted(list(b) + ['d_p']) and all(np.array_equal(a[k], b[k]) for k in b)
    assert a['d_p'].shape == (case['spec']['Q'], 3) and np.abs(a['d_p']).max() > 0


@pytest.mark.parametrize('n_freqs,scale', dc.KERNEL_ENCODINGS)
@pytest.mark.parametrize('second', dc.KERNEL_SECOND)
def test_contract_equals_autograd_of_the_encoding(n_freqs, scale, second):
    """F(p) = <PE(p), t> has dF/dp = J^T t; G(p) = <d_grad, d <PE(p), g> / dp> has dG/dp = H[g, d_grad]."""
    n = 37
    inp = dc.kernel_inputs(n, n_freqs, 64, 40, second)
    kw = dc.kernel_views(inp, n_freqs)
    d_pe = 3 + 6 * n_freqs
    p = kw['p'].double().requires_grad_(True)
    t = (kw['dz0'].double() @ kw['w0'].double() + kw['dzs'].double() @ kw['ws'].double()).detach()
    obj = (ec.encode(p, n_freqs, scale) * t).sum()
    if second != 'none':
        g = kw['g_pe'].double() + (kw['g_pe2'].double() if second == 'two' else 0.0)
        inner = torch.autograd.grad((ec.encode(p, n_freqs, scale) * g[:, :d_pe]).sum(), p, create_graph=True)[0]
        obj = obj + (inner * kw['d_grad'].double()).sum()
    obj.backward()
    got = dc.point_grad_contract(n_freqs=n_freqs, scale=scale, **kw)
    assert _rel(got, p.grad.numpy()) <= 1e-12
    got32 = dc.point_grad_contract(n_freqs=n_freqs, scale=scale, dtype=np.float32, **kw)
    assert got32.dtype == np.float32 and _rel(got32.astype(np.float64), got) <= 1e-4
