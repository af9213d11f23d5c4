"""The float64 definitions of tests/engine_cases.py checked against the oracle's own modules, and the properties of the cases that
tests/test_engines_gpu.py relies on: every case keeps the ReLU-kink cap, the jvp definition is the derivative of the encoding, the
torch-indexing statement of scatter / gather round-trips."""
import copy

import numpy as np
import pytest
import torch

from oracle import stage1 as o1
from oracle import stage2 as o2
from tests import engine_cases as ec
from tests.helpers import stage1_cfg, stage1_state_dict, stage2_state_dict


def _close64(a, b, name, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, '%s: %s vs %s' % (name, tuple(a.shape), tuple(b.shape))
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err <= tol, '%s: %.3e of the largest entry' % (name, err)


def test_visibility_definition_is_the_oracle_module_in_float64():
    conf = o2.bear_conf()
    net = o2.PSNetwork(conf)
    net.load_state_dict(stage2_state_dict(conf, seed=31))
    vn = copy.deepcopy(net.visibility_net).double()
    Ws, bs = ec.vis_weights()
    assert all(torch.equal(m.weight.float(), w) and torch.equal(m.bias.float(), b) for m, w, b in zip(vn.linears, Ws, bs))
    spec = (130, 1, 3)
    Ns, L, V = spec
    x, l = ec.vis_points(spec)
    with torch.no_grad():
        inp = torch.cat([o2.embed(x.double(), ec.VIS_FREQS).tile(L + V, 1), o2.embed(l.double(), ec.VIS_FREQS).repeat_interleave(Ns, dim=0)], -1)
        want = vn(inp)
        rows = ec.vis_rows(ec.pe_table(x.double(), ec.VIS_FREQS), ec.pe_table(l.double(), ec.VIS_FREQS))
        _close64(rows, inp, 'expanded rows')
        got, zs = ec.relu_mlp(rows, [w.double() for w in Ws], [b.double() for b in bs], ec.VIS_SKIP_AT)
    assert len(zs) == 8 and all(z.shape == ((L + V) * Ns, 256) for z in zs)
    _close64(got, want, 'visibility net')


def test_appearance_definition_is_the_oracle_module_in_float64():
    cfg = stage1_cfg('bear')
    net = o1.NeuralNetwork(cfg)
    net.load_state_dict(stage1_state_dict(cfg, seed=21))
    Ws, bs, d_x, n_freqs = ec.app_weights('bear')
    assert (d_x, n_freqs) == (3 + (3 + 6 * net.octaves_pe_views) + 3, net.octaves_pe_views) and len(Ws) == net.n_app
    spec = (130, 'bear')
    p, v, nrm, feat, x = ec.app_points(spec)
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        vh = v.double() / torch.norm(v.double(), dim=-1, keepdim=True)
        want = net64.infer_app(p.double(), nrm.double()[:, None], o1.positional_encoding(vh, n_freqs), feat.double())
        W64 = [getattr(net64, 'lina%d' % l).weight() for l in range(net.n_app)]
        x64 = torch.cat([p.double(), ec.encode(vh, n_freqs)], -1)
        y, zs = ec.app_forward(x64, nrm.double(), feat.double(), W64, [b.double() for b in bs])
    assert len(zs) == 4 and x64.shape[1] == d_x - 3
    _close64(torch.tanh(y) * 0.5 + 0.5, want, 'appearance net')
    # the float32 table of the case is that input in float32: v / |v| carries ~2 ulp (1.2e-7), which the top band multiplies by 2^3
    _close64(x[:, :d_x], torch.cat([x64, nrm.double()], -1), 'input table', 8 * 1.2e-7 + 1.2e-7)
    assert not x[:, d_x:].any()


def test_effective_matrices_are_what_the_networks_hand_to_the_packers():
    """engine_cases states w = v (g / |v|) (and the skip layer's 1 / sqrt(2)) with the oracle's module; NeuralNetwork._app_params /
    _geo_params evaluate the same expressions on the host: equal bit for bit."""
    from psnerf_amd.stage1 import NeuralNetwork
    cfg = stage1_cfg('bear')
    net = NeuralNetwork(cfg)
    net.load_state_dict(stage1_state_dict(cfg, seed=21))
    with torch.no_grad():
        Ws, bs = net._app_params()
        geo = net._geo_params()
    for l, (a, b) in enumerate(zip(Ws + bs, ec.app_weights('bear')[0] + ec.app_weights('bear')[1])):
        assert torch.equal(a, b), 'appearance parameter %d' % l
    params, octaves, skips, scale = ec.geo_weights()
    assert (octaves, skips, scale) == (net.octaves_pe, tuple(net.skips), 1.0 / net.rescale) and len(params) == len(geo)
    for l, (a, b) in enumerate(zip(geo, params)):
        assert torch.equal(a, b), 'geometry parameter %d' % l


def test_geometry_definition_is_the_oracle_module_in_float64():
    cfg = stage1_cfg('bear')
    net = o1.NeuralNetwork(cfg)
    net.load_state_dict(stage1_state_dict(cfg, seed=21))
    net64 = copy.deepcopy(net).double()
    _, octaves, skips, scale = ec.geo_weights()
    inv = 1.0 / np.sqrt(2)
    P64 = []
    with torch.no_grad():
        for l in range(net.n_geo):
            lin = getattr(net64, 'lin%d' % l)
            P64 += [lin.weight() * inv if l in net.skips else lin.weight(), lin.bias.detach()]
    pts = ec.geo_case(ec.GEO_CASES[2])['pts'].double()
    logit, feat, grad = ec.geo_field(pts.clone().requires_grad_(True), P64, octaves, skips, scale)
    want = net64.infer_occ(pts)
    _close64(logit, want[:, :1], 'logit')
    _close64(feat, want[:, 1:], 'features')
    _close64(grad, net64.gradient(pts.clone(), tflag=False)[:, 0], 'd logit / d p')
    # the float32 effective matrices of the cases are these, rounded
    for a, b in zip(ec.geo_weights()[0], P64):
        _close64(a, b, 'effective parameter', 3e-7)


@pytest.mark.parametrize('spec', ec.VIS_CASES, ids=ec.vis_id)
def test_visibility_cases_keep_the_kink_cap(spec):
    c = ec.vis_case(spec)
    Ns, L, V = spec
    print('%s: eps %.2e, %d of %d supervised rows masked' % (ec.vis_id(spec), c['eps'], int(c['masked'].sum()), V * Ns))
    assert c['masked'].shape == (V * Ns,) and 0.0 < c['eps'] < 1e-5
    assert c['share'] <= ec.KINK_CAP
    assert not c['c'][c['masked']].any() and bool((c['c'][~c['masked']] != 0).all())


@pytest.mark.parametrize('spec', ec.APP_CASES, ids=ec.app_id)
def test_appearance_cases_keep_the_kink_cap(spec):
    c = ec.app_case(spec)
    print('%s: eps %.2e, %d of %d rows masked' % (ec.app_id(spec), c['eps'], int(c['masked'].sum()), spec[0]))
    assert c['masked'].shape == (spec[0],) and 0.0 < c['eps'] < 2e-5
    assert c['share'] <= ec.KINK_CAP
    assert not c['c'][c['masked']].any() and bool((c['c'][~c['masked']] != 0).all())
    assert torch.equal(c['normal'], c['x'][:, c['d_x'] - 3:c['d_x']])


def test_masked_rows_reach_no_reference_gradient():
    """Zero upstream gradient on a row = the row contributes to no parameter gradient: the float64 gradients of a case equal those of
    the case with its masked rows REMOVED."""
    spec = (333, 2, 3)
    c = ec.vis_case(spec)
    assert int(c['masked'].sum()) > 0
    ref = ec.vis_reference(c, torch.float64)
    Ns, L, V = spec
    Ws, bs = (ec._leaves(t, torch.float64) for t in ec.vis_weights())
    rows = ec.vis_rows(c['pe_x'], c['pe_l'])[L * Ns:][~c['masked']].double()
    out, _ = ec.relu_mlp(rows, Ws, bs, ec.VIS_SKIP_AT)
    (out * c['c'][~c['masked']].double()).sum().backward()
    for l in range(len(Ws)):
        _close64(torch.from_numpy(ref['dW%d' % l]), Ws[l].grad, 'dW%d' % l)
        _close64(torch.from_numpy(ref['db%d' % l]), bs[l].grad, 'db%d' % l)


def test_geometry_cases_cover_the_forms_the_trainer_runs():
    ids = [ec.geo_id(s) for s in ec.GEO_CASES]
    assert len(set(ids)) == len(ids)
    assert {s['Q'] for s in ec.GEO_CASES if s['feat_rows'] is None and s['with_grad'] and len(s['use']) == 3} == {1, 65, 130, 1000}
    assert {s['feat_rows'] for s in ec.GEO_CASES if s['Q'] == 1000 and s['with_grad']} == {None, 1, 63, 64, 999}
    assert any(not s['with_grad'] for s in ec.GEO_CASES)
    assert {tuple(s['use']) for s in ec.GEO_CASES if s['with_grad'] and len(s['use']) == 2} == {
        ('feat', 'grad'), ('logit', 'grad'), ('logit', 'feat')}
    c = ec.geo_case(ec.GEO_CASES[5])
    r = ec.geo_reference(c, torch.float64)
    assert r['feat'].shape == (63, 256) and r['grad'].shape == (1000, 3) and r['dW0'].shape == (256, 39)
    assert all(np.abs(r[k]).max() > 0 for k in r)


@pytest.mark.parametrize('n_freqs,scale', [(0, 1.0), (6, 1.0), (6, 0.5), (10, 0.5)])
def test_jvp_definition_is_the_derivative_of_the_encoding(n_freqs, scale):
    x, t = ec.pe_jvp_inputs(63, n_freqs, scale)
    jv = ec.pe_jvp(x, t, n_freqs, scale)
    width = 3 + 6 * n_freqs
    assert jv.shape == (63, 64) and jv.dtype == torch.float64 and not jv[:, width:].any()
    h = 1e-4 / 2.0 ** n_freqs
    x64, t64 = x.double(), t.double()
    fd = (ec.encode(x64 + h * t64, n_freqs, scale) - ec.encode(x64 - h * t64, n_freqs, scale)) / (2 * h)
    # central difference, relative to the top band's 2^F: truncation (2^F h)^2 / 6 = 1.7e-9, rounding of the argument 2^F x in float64
    # 1e-16 2^F / (2^F h) = 1e-9 at F = 10
    _close64(jv[:, :width], fd, 'jvp vs central difference', 1e-8)
    assert ec.pe_table(x, n_freqs, scale).shape == (63, 64) and not ec.pe_table(x, n_freqs, scale)[:, width:].any()


@pytest.mark.parametrize('shape', ec.SCATTER_SHAPES, ids=ec.scatter_id)
def test_scatter_definition_round_trips(shape):
    n_pix, ns = shape
    idx, rows, grads = ec.scatter_inputs(n_pix, ns)
    assert idx.shape == (ns,) and bool((idx[1:] > idx[:-1]).all()) and len(ec.SCATTER_SPECS) == 17
    assert {s[0] for s in ec.SCATTER_SPECS} == {1, 3} and {s[1] for s in ec.SCATTER_SPECS} == {1, 3, 9}
    assert {s[2] for s in ec.SCATTER_SPECS} == {0.0, 1.0, -2.5}
    dense = ec.scatter_dense(ec.SCATTER_SPECS, rows, idx, n_pix)
    back = ec.gather_dense(ec.SCATTER_SPECS, dense, idx)
    off = torch.ones(n_pix, dtype=torch.bool)
    off[idx] = False
    for (B, C, fill), d, r, b in zip(ec.SCATTER_SPECS, dense, rows, back):
        assert d.shape == (B, n_pix, C) and torch.equal(b, r.contiguous())
        assert bool((d[:, off] == fill).all())
    # the adjoint identity <scatter(rows), g> = <rows, gather(g)> + fill terms, on one output
    B, C, fill = ec.SCATTER_SPECS[3]
    lhs = (dense[3].double() * grads[3].double()).sum()
    rhs = (rows[3].double() * ec.gather_dense(ec.SCATTER_SPECS, grads, idx)[3].double()).sum() + fill * grads[3][:, off].double().sum()
    assert abs(float(lhs - rhs)) <= 1e-9 * max(1.0, abs(float(lhs)))
    # a padded list: only the first of equal entries is live
    if ns > 1:
        padded = torch.cat([idx, idx[-1:].expand(3)])
        live = torch.cat([torch.ones(ns, dtype=torch.bool), torch.zeros(3, dtype=torch.bool)])
        got = ec.gather_dense(ec.SCATTER_SPECS[:2], grads[:2], padded, live=live)
        for k, ((B, C, _), g) in enumerate(zip(ec.SCATTER_SPECS[:2], got)):
            g = g.view(B, ns + 3, C)
            assert not g[:, ns:].any() and torch.equal(g[:, :ns], grads[k][:, idx])
