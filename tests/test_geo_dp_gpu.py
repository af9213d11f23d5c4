"""d loss / d p of the stage-1 geometry field on the device: psn_geo_point_grad alone against the numpy float64 statement of its
contract (tests/geo_dp_cases.py), the two engines (ops.GeoFieldFused at every spec of engine_cases.GEO_CASES, ops.GeoField) with
pts.requires_grad_() against the float64 definition extended by pts.grad, and psnerf_amd.stage1.NeuralNetwork against the oracle
network.  Plus what must NOT move: with p requiring a gradient every output and parameter gradient keeps its bits, and with no
parameter requiring one d_p keeps its bits while no weight-gradient launch is made.

Tolerance: none chosen -- the rule of tests/test_engines_gpu.py.  Per tensor, bound = 1e-5 |truth| + 1e-5 max|truth|; r_ref = the
definition in float32 on the CPU against truth, r_hip = the device against truth, both in units of the bound; the device may have as
many elements beyond the bound as the reference arithmetic has beyond half of it, and a worst element of max(1, 2 max r_ref).

Measured on an MI355X (gfx950), worst case over all cases, in units of the bound: r_hip (r_ref of the same case).
    kernel alone    d_p 0.080 (0.030)   d_p with the second-order group 0.061 (0.012)
    GeoFieldFused   d_p 0.113 (0.076)   [with_grad = False: 0.030 (0.028)]
                    every other tensor as in tests/test_engines_gpu.py: logit 0.069 (0.049), feat 0.152 (0.060), grad 0.056 (0.034),
                    dW at most 0.248 (0.210), db at most 0.246 (0.127)
    GeoField        d_p 0.120 (0.064)   [with_grad = False: 0.046 (0.018)]   logit 0.067 (0.032), feat 0.090 (0.046), grad 0.056 (0.043),
                    dW at most 0.208 (0.186), db at most 0.178 (0.134)
    NeuralNetwork   only_occupancy: out 0.050 (0.045), d_p 0.082 (0.073); return_logits within those figures
Every tensor stays inside the plain bound; the allowance is not drawn on.
"""
import numpy as np
import pytest
import torch

from tests import engine_cases as ec
from tests import geo_dp_cases as dc
from tests.helpers import assert_vs_truth, stage1_cfg, stage1_state_dict

pytestmark = pytest.mark.gpu
RTOL = 1e-5
_WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _WORST:
        print('\n==== point gradient vs float64: worst r_hip (the reference arithmetic in the same case) ====')
        for (group, name), (rh, rr, where) in sorted(_WORST.items()):
            print('%-10s %-8s r_hip %7.3f  r_ref %7.3f  (%s)' % (group, name, rh, rr, where))


def check(group, where, name, got, ref, truth):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == truth.shape, '%s %s %s: shape %s vs %s' % (group, where, name, got.shape, truth.shape)
    rh, rr = assert_vs_truth('%s %s %s' % (group, where, name), got, ref, truth, RTOL, 'max')
    if rh > _WORST.get((group, name), (-1.0,))[0]:
        _WORST[(group, name)] = (rh, rr, where)


# --------------------------------------------------------------------------- the kernel alone
def kernel_call(inp, n_freqs, scale, cuda):
    from psnerf_amd import hip
    kw = dc.kernel_views({k: t.to(cuda) for k, t in inp.items()}, n_freqs)
    assert all(t.stride(0) > t.shape[1] for k, t in kw.items() if k not in ('p', 'd_grad'))
    return hip.geo_point_grad(kw.pop('p'), n_freqs, scale, kw.pop('dz0'), kw.pop('w0'), **kw)


@pytest.mark.parametrize('h0,hs', dc.KERNEL_WIDTHS, ids=lambda v: 'x' if v is None else str(v))
@pytest.mark.parametrize('n_freqs,scale', dc.KERNEL_ENCODINGS)
def test_point_grad_kernel_vs_float64_contract(cuda, n_freqs, scale, h0, hs):
    for n in dc.KERNEL_ROWS:
        for second in dc.KERNEL_SECOND:
            inp = dc.kernel_inputs(n, n_freqs, h0, hs, second)
            got = kernel_call(inp, n_freqs, scale, cuda)
            kw = dc.kernel_views(inp, n_freqs)
            truth = dc.point_grad_contract(n_freqs=n_freqs, scale=scale, **kw)
            ref = dc.point_grad_contract(n_freqs=n_freqs, scale=scale, dtype=np.float32, **kw)
            where = 'n%d-f%d-s%g-h%d+%s-%s' % (n, n_freqs, scale, h0, hs, second)
            check('kernel', where, 'd_p' if second == 'none' else 'd_p+H', got, ref, truth)


def test_point_grad_kernel_empty_input_and_determinism(cuda):
    from psnerf_amd import hip
    inp = dc.kernel_inputs(1000, 6, 256, 256, 'two')
    a, b = kernel_call(inp, 6, 1.0, cuda), kernel_call(inp, 6, 1.0, cuda)
    assert torch.equal(a, b)
    z = lambda r, c: torch.zeros(r, c, device=cuda)
    out = hip.geo_point_grad(z(0, 3), 6, 1.0, z(0, 256), z(256, 39), dzs=z(0, 256), ws=z(256, 39), g_pe=z(0, 64), d_grad=z(0, 3))
    assert out.shape == (0, 3)
    with pytest.raises(RuntimeError, match='geo_point_grad'):   # 3 + 6 * 11 columns do not fit
        hip.geo_point_grad(z(4, 3), 11, 1.0, z(4, 8), z(8, 69))


# --------------------------------------------------------------------------- the engines
def leaves(ts, cuda, requires_grad=True):
    return [t.to(cuda).requires_grad_(requires_grad) for t in ts]


def param_grads(params):
    out = {}
    for l in range(len(params) // 2):
        out['dW%d' % l], out['db%d' % l] = params[2 * l].grad, params[2 * l + 1].grad
    return out


def engine_run(spec, cuda, fused_engine=True, p_grad=True, w_grad=True):
    """-> {name: device tensor}: the outputs, 'd_p' (p_grad) and the parameter gradients (w_grad) of geo_objective."""
    from psnerf_amd import fused, ops
    case = ec.geo_case(spec)
    params_host, octaves, skips, scale = ec.geo_weights()
    params = leaves(params_host, cuda, w_grad)
    pts = case['pts'].detach().to(cuda).requires_grad_(p_grad)
    if fused_engine:
        chains = fused.pack_geo_chains(params[0::2], params[1::2], list(skips), 3 + 6 * octaves)
        logit, feat, grad = ops.GeoFieldFused.apply(pts, octaves, scale, skips, spec['with_grad'], chains, spec['feat_rows'], *params)
    else:
        assert spec['feat_rows'] is None
        out, grad = ops.GeoField.apply(pts, octaves, scale, skips, spec['with_grad'], *params)
        logit, feat = out[:, :1], out[:, 1:]
    ec.geo_objective(case, logit, feat, grad).backward()
    got = dict(logit=logit.detach(), feat=feat.detach(), grad=grad.detach())
    if p_grad:
        assert pts.grad is not None, 'the engine returned no gradient for p'
        got['d_p'] = pts.grad
    if w_grad:
        got.update(param_grads(params))
    return got


def engine_check(group, spec, got):
    case = ec.geo_case(spec)
    r32, r64 = dc.geo_reference_dp(case, torch.float32), dc.geo_reference_dp(case, torch.float64)
    if not spec['with_grad']:   # the engine's grad output is a non-differentiable zero: no second-order term in d_p
        assert not got.pop('grad').any()
        r32, r64 = ({k: v for k, v in r.items() if k != 'grad'} for r in (r32, r64))
    assert sorted(got) == sorted(r64), (sorted(got), sorted(r64))
    for name in sorted(got):
        check(group, ec.geo_id(spec), name, got[name], r32[name], r64[name])


@pytest.mark.parametrize('spec', ec.GEO_CASES, ids=ec.geo_id)
def test_geo_field_fused_point_gradient_vs_float64(cuda, spec):
    engine_check('fused' if spec['with_grad'] else 'fused-ng', spec, engine_run(spec, cuda))


@pytest.mark.parametrize('spec', dc.GEOFIELD_CASES, ids=ec.geo_id)
def test_geo_field_layerwise_point_gradient_vs_float64(cuda, spec):
    engine_check('layer' if spec['with_grad'] else 'layer-ng', spec, engine_run(spec, cuda, fused_engine=False))


@pytest.mark.parametrize('fused_engine', [True, False], ids=['fused', 'layerwise'])
@pytest.mark.parametrize('Q', [130, 1000])
def test_nothing_else_moves_when_p_requires_a_gradient(cuda, Q, fused_engine):
    spec = dict(Q=Q, feat_rows=None, with_grad=True, use=ec._ALL)
    a, b = engine_run(spec, cuda, fused_engine, p_grad=True), engine_run(spec, cuda, fused_engine, p_grad=False)
    a.pop('d_p')
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), '%s changed its bits' % k


@pytest.mark.parametrize('fused_engine', [True, False], ids=['fused', 'layerwise'])
def test_no_weight_gradient_launch_when_no_parameter_needs_one(cuda, monkeypatch, fused_engine):
    from psnerf_amd import hip
    spec = dict(Q=130, feat_rows=None, with_grad=True, use=ec._ALL)
    with_w = engine_run(spec, cuda, fused_engine)
    calls = []
    real_gemm = hip.gemm
    monkeypatch.setattr(hip, 'gemm_tn_grouped', lambda *a, **k: calls.append('gemm_tn_grouped'))
    monkeypatch.setattr(hip, 'colsum', lambda *a, **k: calls.append('colsum'))
    monkeypatch.setattr(hip, 'gemm', lambda *a, **k: calls.append('gemm trans_a') if k.get('trans_a') else real_gemm(*a, **k))
    without = engine_run(spec, cuda, fused_engine, w_grad=False)
    assert calls == []
    assert torch.equal(without['d_p'], with_w['d_p'])
    for k in ('logit', 'feat', 'grad'):
        assert torch.equal(without[k], with_w[k])


# --------------------------------------------------------------------------- the network
def _networks(cuda):
    from oracle import stage1 as o1
    from psnerf_amd.stage1 import NeuralNetwork
    cfg = stage1_cfg('bear')
    sd = stage1_state_dict(cfg, seed=21)
    net = NeuralNetwork(cfg)
    net.load_state_dict(sd)
    onet = o1.NeuralNetwork(cfg)
    onet.load_state_dict(sd)
    return net.to(cuda), onet


@pytest.mark.parametrize('mode', ['only_occupancy', 'return_logits'])
def test_network_point_gradient_vs_oracle(cuda, mode):
    net, onet = _networks(cuda)
    pts = ec.geo_case(dict(Q=130, feat_rows=None, with_grad=True, use=ec._ALL))['pts'].detach()
    p = pts.to(cuda).requires_grad_(True)
    out = net(p[None], None, **{mode: True})
    out.sum().backward()
    assert p.grad is not None, 'the network call is not differentiable in p'
    refs = []
    for dtype in (torch.float32, torch.float64):
        q = pts.detach().clone().to(dtype).requires_grad_(True)
        o = onet.to(dtype)(q[None], None, **{mode: True})
        o.sum().backward()
        refs.append((o.detach().double().numpy(), q.grad.double().numpy()))
    check('network', mode, 'out', out, refs[0][0], refs[1][0])
    check('network', mode, 'd_p', p.grad, refs[0][1], refs[1][1])


def test_network_render_path_stays_non_differentiable_in_p(cuda):
    net, _ = _networks(cuda)
    case = ec.geo_case(dict(Q=130, feat_rows=None, with_grad=True, use=ec._ALL))
    p = case['pts'].detach().to(cuda).requires_grad_(True)
    ray_d = torch.nn.functional.normalize(case['c_grad'], dim=-1).to(cuda)
    rgb = net(p[None], ray_d[None])
    rgb.sum().backward()
    assert p.grad is None
    assert net.lin0.weight_v.grad is not None
    q = case['pts'].detach().to(cuda).requires_grad_(True)
    rgb2, occ, g = net.render_and_gradient(q[None], ray_d[None], q[:7])
    (rgb2.sum() + occ.sum() + g.sum()).backward()
    assert q.grad is None
