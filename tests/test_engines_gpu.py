"""The three fused autograd engines -- ops.VisibilityPair (stage-2 visibility net, both row groups in one launch), ops.AppNetFused
(stage-1 appearance net) and ops.GeoFieldFused (stage-1 geometry field with its gradient sweep) -- forward AND hand-derived backward
against the float64 definitions of tests/engine_cases.py, tensor by tensor; and the two kernels under them that had no test:
psn_pe_encode_jvp against torch.autograd.functional.jvp of the float64 encoding, psn_scatter_rows / psn_gather_rows /
psn_gather_rows_valid (ops.ScatterRows) against torch indexing, bit for bit.

Inputs are shared: the encoded tables are written on the device (hip.pe_encode / hip.app_input), read back, and both reference
evaluations start from those float32 values; the effective weight matrices are formed on the host.  ReLU kinks are handled by the
reference alone (engine_cases: eps = 4 x max |z_fp32 - z_float64|, zero upstream gradient on every row with a hidden |z_float64| <= eps,
at most 5 % of a case's rows -- asserted here on the device-written tables as well as in tests/test_engines_cpu.py).

Tolerance: none chosen.  Per tensor, bound = 1e-5 |truth| + 1e-5 max|truth|; r_ref = the definition in float32 on the CPU against
truth, r_hip = the engine against truth, both in units of the bound.  The engine may have as many elements beyond the bound as the
reference arithmetic has beyond half of it, and its worst element may be max(1, 2 max r_ref) (tests/helpers.py).

Measured on an MI355X (gfx950), worst case over all cases, in units of the bound: r_hip (r_ref of the same case).  Every tensor of
every engine stays inside the plain bound; the allowance is not drawn on.
    VisibilityPair  vis 0.081 (0.055)   vis_t 0.086 (0.061)
                    dW0..dW8  0.055 (0.053)  0.066 (0.051)  0.083 (0.043)  0.115 (0.051)  0.077 (0.047)  0.029 (0.029)  0.060 (0.035)
                              0.085 (0.047)  0.113 (0.167)
                    db0..db8  0.058 (0.040)  0.058 (0.029)  0.068 (0.049)  0.054 (0.037)  0.051 (0.036)  0.052 (0.024)  0.037 (0.027)
                              0.040 (0.029)  0.032 (0.050)
    AppNetFused     y 0.056 (0.011)   d_normal 0.127 (0.055)   d_feat 0.037 (0.031)
                    dW0..dW4  0.051 (0.029)  0.056 (0.027)  0.050 (0.027)  0.041 (0.029)  0.060 (0.026)
                    db0..db4  0.044 (0.025)  0.030 (0.026)  0.025 (0.022)  0.012 (0.010)  0.006 (0.004)
    GeoFieldFused   logit 0.069 (0.049)   feat 0.152 (0.060)   grad 0.056 (0.034)        [with_grad = False: logit 0.052, feat 0.067]
                    dW0..dW8  0.144 (0.100)  0.173 (0.130)  0.228 (0.131)  0.248 (0.210)  0.076 (0.049)  0.181 (0.100)  0.188 (0.116)
                              0.215 (0.186)  0.132 (0.106)                               [with_grad = False: at most 0.206 (0.165)]
                    db0..db8  0.153 (0.110)  0.169 (0.111)  0.246 (0.127)  0.215 (0.139)  0.164 (0.079)  0.161 (0.110)  0.128 (0.089)
                              0.216 (0.103)  0.036 (0.062)                               [with_grad = False: at most 0.192 (0.141)]
                    the double-backward gradients carry the softplus beta = 100 and are the largest figures here -- in the reference
                    arithmetic as much as in the chains (r_ref up to 0.21): still a quarter of the plain bound.
    pe_encode_jvp   0.004 (0.003)
eps and masked rows per case, on the device-written tables (the CPU of the GPU machine; tests/test_engines_cpu.py prints the host's):
    VisibilityPair  Ns1-L1-V1 7.3e-07, 0 of 1      Ns63-L1-V2 3.1e-06, 3 of 126      Ns64-L2-V1 2.9e-06, 1 of 64
                    Ns130-L1-V3 2.8e-06, 9 of 390   Ns333-L2-V3 3.5e-06, 28 of 999    Ns128-L3-V16 4.1e-06, 53 of 2048
                    Ns96-L1-V17 3.9e-06, 43 of 1632
    AppNetFused     Q1 7.6e-07, 0    Q63 1.7e-06, 0    Q64 1.8e-06, 0    Q65 2.0e-06, 1    Q130 2.1e-06, 3    Q1000 2.5e-06, 23
                    Q130-full (d_x = 64) 3.9e-06, 0
eps comes out at 2 - 4e-6, not below 1e-6: layer 0 of the visibility net sums 126 products through partial sums of up to 2, and its
float32 value differs from float64 by up to 9e-7 in any summation order.  At that margin randomly drawn points mask 6 - 8 % of the rows,
so engine_cases draws the points by rejection (at most 3 % of a case's rows near a kink); the cap itself stands.
"""
import numpy as np
import pytest
import torch

from tests import engine_cases as ec
from tests.helpers import assert_vs_truth

pytestmark = pytest.mark.gpu
RTOL = 1e-5
_WORST = {}   # (engine, tensor) -> (worst r_hip, r_ref of that case, case)
_NOTES = {}   # (engine, case) -> eps and masked share on the device-written tables


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _WORST:
        print('\n==== fused engines vs float64: worst r_hip (the reference arithmetic in the same case) ====')
        for (engine, name), (rh, rr, where) in sorted(_WORST.items()):
            print('%-6s %-10s r_hip %7.3f  r_ref %7.3f  (%s)' % (engine, name, rh, rr, where))
        for (engine, where), note in sorted(_NOTES.items()):
            print('%-6s %-28s %s' % (engine, where, note))


def check(engine, where, name, got, ref, truth):
    """One tensor of one case against truth under the measured allowance; records the worst figures per engine and tensor."""
    got = got.detach().cpu().numpy()
    assert got.shape == truth.shape, '%s %s %s: shape %s vs %s' % (engine, where, name, got.shape, truth.shape)
    rh, rr = assert_vs_truth('%s %s %s' % (engine, where, name), got, ref, truth, RTOL, 'max')
    if rh > _WORST.get((engine, name), (-1.0,))[0]:
        _WORST[(engine, name)] = (rh, rr, where)


def check_all(engine, where, got, ref32, ref64):
    """got: {name: device tensor} -- every name of the reference must be there."""
    assert sorted(got) == sorted(ref64), (sorted(got), sorted(ref64))
    for name in sorted(got):
        check(engine, where, name, got[name], ref32[name], ref64[name])


def leaves(ts, cuda):
    return [t.to(cuda).requires_grad_() for t in ts]


def interleave(Ws, bs):
    return [t for pair in zip(Ws, bs) for t in pair]


def param_grads(params):
    out = {}
    for l in range(len(params) // 2):
        out['dW%d' % l], out['db%d' % l] = params[2 * l].grad, params[2 * l + 1].grad
    return out


def same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), '%s: %s differs' % (what, k)


# --------------------------------------------------------------------------- VisibilityPair
_VIS = {}


def vis_on_device(spec, cuda):
    """(case on the device-written tables, pe_x, pe_l).  Cached: the references are computed once per case."""
    if spec not in _VIS:
        from psnerf_amd import hip
        x, l = ec.vis_points(spec)
        pe_x, pe_l = hip.pe_encode(x.to(cuda), ec.VIS_FREQS, 64), hip.pe_encode(l.to(cuda), ec.VIS_FREQS, 64)
        for dev, host in ((pe_x, ec.pe_table(x, ec.VIS_FREQS)), (pe_l, ec.pe_table(l, ec.VIS_FREQS))):
            # sinf / cosf against torch's float32 sin / cos of the same (exactly scaled) argument: two ulp of 1.0 each
            assert float((dev.cpu() - host).abs().max()) <= 4 * 2.0 ** -23 and not dev[:, 63:].any()
        case = ec.vis_case(spec, pe_x, pe_l)
        _NOTES[('vis', ec.vis_id(spec))] = 'eps %.2e, masked %d of %d supervised rows' % (case['eps'], int(case['masked'].sum()), case['masked'].numel())
        assert case['share'] <= ec.KINK_CAP, _NOTES[('vis', ec.vis_id(spec))]
        _VIS[spec] = (case, pe_x, pe_l)
    return _VIS[spec]


def vis_cols(cuda, contiguous_attr=True):
    """in_cols as PSNetwork._cols(.., pair=True) builds it."""
    c = torch.arange(ec.VIS_DIN_HALF, device=cuda)
    c = torch.cat([c, 64 + c])
    if contiguous_attr:
        c._psn_contiguous_pair = True
    return c


def vis_run(spec, cuda, cols=None, prelaunch=False):
    """-> (vis, vis_t, {dW_l, db_l}) of (vis_t * c).sum()."""
    from psnerf_amd import ops
    case, pe_x, pe_l = vis_on_device(spec, cuda)
    Ns, L, V = spec
    params = leaves(interleave(*ec.vis_weights()), cuda)
    cols = vis_cols(cuda) if cols is None else cols
    pre = None
    if prelaunch:
        pre = ops.VisibilityPair.launch(pe_x, pe_l, L, cols, ec.VIS_SKIP_AT, [p.detach() for p in params], True)
    vis, vis_t = ops.VisibilityPair.apply(pe_x, pe_l, L, cols, ec.VIS_SKIP_AT, pre, *params)
    assert vis.shape == (L * Ns, 1) and vis_t.shape == (V * Ns, 1)
    assert not vis.requires_grad and vis_t.requires_grad   # the shading rows enter the loss detached
    (vis_t * case['c'].to(cuda)).sum().backward()
    return vis.detach(), vis_t.detach(), param_grads(params)


@pytest.mark.parametrize('spec', ec.VIS_CASES, ids=ec.vis_id)
def test_visibility_pair_vs_float64(cuda, spec):
    vis, vis_t, grads = vis_run(spec, cuda)
    case = vis_on_device(spec, cuda)[0]
    got = dict(grads, vis=vis, vis_t=vis_t)
    check_all('vis', ec.vis_id(spec), got, ec.vis_reference(case, torch.float32), ec.vis_reference(case, torch.float64))


def test_visibility_pair_column_index_path_is_bit_identical(cuda):
    """The same in_cols values WITHOUT the _psn_contiguous_pair attribute (index kernels instead of slices)."""
    spec = (130, 1, 3)
    plain = vis_cols(cuda, contiguous_attr=False)
    assert not hasattr(plain, '_psn_contiguous_pair') and torch.equal(plain, vis_cols(cuda))
    a, b = vis_run(spec, cuda), vis_run(spec, cuda, cols=plain)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    same_bits(a[2], b[2], 'column-index path')


def test_visibility_pair_sign_bits_and_activation_masks_agree(cuda):
    """ops.RELU_SIGN_BITS = False (the activation rows themselves as masks): every gradient bit for bit."""
    from psnerf_amd import ops
    spec = (130, 1, 3)
    assert ops.RELU_SIGN_BITS
    a = vis_run(spec, cuda)
    ops.RELU_SIGN_BITS = False
    try:
        b = vis_run(spec, cuda)
    finally:
        ops.RELU_SIGN_BITS = True
    assert torch.equal(a[1], b[1])
    same_bits(a[2], b[2], 'activation rows as masks')


def test_visibility_pair_prelaunch_and_determinism(cuda):
    """launch(...) followed by apply(..., pre, ...) equals the direct apply; two runs give identical bits."""
    spec = (333, 2, 3)
    a, b, c = vis_run(spec, cuda), vis_run(spec, cuda), vis_run(spec, cuda, prelaunch=True)
    for other, what in ((b, 'second run'), (c, 'pre-launched')):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1]), what
        same_bits(a[2], other[2], what)


def test_visibility_pair_unused_vis_t_gives_no_parameter_gradients(cuda):
    from psnerf_amd import ops
    spec = (63, 1, 2)
    case, pe_x, pe_l = vis_on_device(spec, cuda)
    params = leaves(interleave(*ec.vis_weights()), cuda)
    vis, vis_t = ops.VisibilityPair.apply(pe_x, pe_l, spec[1], vis_cols(cuda), ec.VIS_SKIP_AT, None, *params)
    # a loss that reaches the parameters by another way and the network's output only through the detached shading rows
    (float(vis.sum()) * params[1].sum()).backward()
    assert all(p.grad is None for i, p in enumerate(params) if i != 1)
    assert torch.equal(params[1].grad, torch.full_like(params[1], float(vis.sum())))
    # the node itself, asked with no gradient for vis_t
    got = ops.VisibilityPair.backward(vis_t.grad_fn, None, None)
    assert len(got) == 6 + len(params) and all(g is None for g in got)


# --------------------------------------------------------------------------- AppNetFused
_APP = {}


def app_on_device(spec, cuda):
    if spec not in _APP:
        from psnerf_amd import hip
        Q, kind = spec
        p, v, nrm, _, x_host = ec.app_points(spec)
        if kind == 'bear':
            x = hip.app_input(p.to(cuda), v.to(cuda), nrm.to(cuda), ec.app_weights(kind)[3])
            d_x = ec.app_weights(kind)[2]
            assert torch.equal(x[:, :3].cpu(), p) and torch.equal(x[:, d_x - 3:d_x].cpu(), nrm) and not x[:, d_x:].any()
            assert float((x.cpu() - x_host).abs().max()) <= 8 * 1.2e-7 + 1.2e-7   # (test_engines_cpu.py: v / |v| in float32, x 2^3)
        else:
            x = x_host.to(cuda)
        case = ec.app_case(spec, x)
        _NOTES[('app', ec.app_id(spec))] = 'eps %.2e, masked %d of %d rows' % (case['eps'], int(case['masked'].sum()), Q)
        assert case['share'] <= ec.KINK_CAP, _NOTES[('app', ec.app_id(spec))]
        _APP[spec] = (case, x)
    return _APP[spec]


def app_run(spec, cuda, x_requires_grad=False):
    from psnerf_amd import fused, ops
    case, x = app_on_device(spec, cuda)
    Ws, bs, d_x, _ = ec.app_weights(spec[1])
    params = leaves(interleave(Ws, bs), cuda)
    normal, feat = leaves([case['normal'], case['feat']], cuda)
    chains = fused.pack_app_chains(params[0::2], params[1::2], d_x)
    x = x.clone().requires_grad_() if x_requires_grad else x
    y = ops.AppNetFused.apply(x, normal, feat, d_x, chains, *params)
    (y * case['c'].to(cuda)).sum().backward()
    return dict(param_grads(params), y=y.detach(), d_normal=normal.grad, d_feat=feat.grad), x


@pytest.mark.parametrize('spec', ec.APP_CASES, ids=ec.app_id)
def test_app_net_fused_vs_float64(cuda, spec):
    got, _ = app_run(spec, cuda)
    case = app_on_device(spec, cuda)[0]
    assert got['d_normal'].shape == (spec[0], 3)   # the gradient of the normal columns alone
    check_all('app', ec.app_id(spec), got, ec.app_reference(case, torch.float32), ec.app_reference(case, torch.float64))


def test_app_net_fused_input_table_gets_no_gradient_and_is_deterministic(cuda):
    spec = (130, 'bear')
    a, _ = app_run(spec, cuda)
    b, x = app_run(spec, cuda, x_requires_grad=True)
    assert x.requires_grad and x.grad is None
    same_bits(a, b, 'second run')


# --------------------------------------------------------------------------- GeoFieldFused
def geo_run(spec, cuda):
    from psnerf_amd import fused, ops
    case = ec.geo_case(spec)
    params_host, octaves, skips, scale = ec.geo_weights()
    params = leaves(params_host, cuda)
    chains = fused.pack_geo_chains(params[0::2], params[1::2], list(skips), 3 + 6 * octaves)
    logit, feat, grad = ops.GeoFieldFused.apply(case['pts'].to(cuda), octaves, scale, skips, spec['with_grad'], chains, spec['feat_rows'], *params)
    ec.geo_objective(case, logit, feat, grad).backward()
    return dict(param_grads(params), logit=logit.detach(), feat=feat.detach(), grad=grad.detach()), grad


@pytest.mark.parametrize('spec', ec.GEO_CASES, ids=ec.geo_id)
def test_geo_field_fused_vs_float64(cuda, spec):
    """feat_rows < Q (normal points riding behind the render samples), with_grad = False (value_bwd_nosweep) and objectives that leave
    one output unused, next to the plain form."""
    got, grad = geo_run(spec, cuda)
    case = ec.geo_case(spec)
    r32, r64 = ec.geo_reference(case, torch.float32), ec.geo_reference(case, torch.float64)
    assert got['feat'].shape == (case['feat_rows'], 256)
    if not spec['with_grad']:
        assert not grad.requires_grad and grad.shape == (spec['Q'], 3) and not grad.any()
        got.pop('grad')
        r32, r64 = ({k: v for k, v in r.items() if k != 'grad'} for r in (r32, r64))
    else:
        assert grad.requires_grad
    check_all('geo' if spec['with_grad'] else 'geo-ng', ec.geo_id(spec), got, r32, r64)


# --------------------------------------------------------------------------- pe_encode_jvp
@pytest.mark.parametrize('n,n_freqs,scale', ec.PE_JVP_CASES)
def test_pe_encode_jvp_vs_float64(cuda, n, n_freqs, scale):
    from psnerf_amd import hip
    x, t = ec.pe_jvp_inputs(n, n_freqs, scale)
    got = hip.pe_encode_jvp(x.to(cuda), t.to(cuda), n_freqs, 64, scale)
    width = 3 + 6 * n_freqs
    assert got.shape == (n, 64)
    assert not got[:, width:].any(), 'padding columns %d .. 64 must be exact zeros (a chain launch multiplies the whole table)' % width
    truth, ref = ec.pe_jvp(x, t, n_freqs, scale), ec.pe_jvp(x, t, n_freqs, scale, dtype=torch.float32)
    check('jvp', 'n%d-F%d-s%g' % (n, n_freqs, scale), 'jvp', got[:, :width], ref[:, :width].numpy(), truth[:, :width].numpy())
    if n_freqs == 0:   # t * scale: one multiplication
        assert torch.equal(got[:, :3].cpu(), t * scale)


# --------------------------------------------------------------------------- scatter_rows / gather_rows / ScatterRows
def rows_on_device(rows, cuda):
    """The strided views rebuilt on the device with the same strides."""
    out = []
    for i, r in enumerate(rows):
        if i == ec.SCATTER_EXPAND:
            out.append(r[:, :1].contiguous().to(cuda).expand(*r.shape))
        elif i == ec.SCATTER_SLICE:
            out.append(r._base.to(cuda)[:, 1:1 + r.shape[1]])
        else:
            out.append(r.to(cuda))
        assert out[-1].stride() == r.stride() and torch.equal(out[-1].cpu(), r)
    return out


@pytest.mark.parametrize('shape', ec.SCATTER_SHAPES, ids=ec.scatter_id)
def test_scatter_and_gather_rows_are_exact_copies(cuda, shape):
    """17 outputs in one call (two launches), B in {1, 3}, C in {1, 3, 9}, fills 0 / 1 / -2.5, a stride-0 column and a column slice."""
    from psnerf_amd import hip
    n_pix, ns = shape
    specs = list(ec.SCATTER_SPECS)
    assert len(specs) > hip.SCATTER_MAX_ITEMS
    idx, rows, grads = ec.scatter_inputs(n_pix, ns)
    idx_d, grads_d = idx.to(cuda), [g.to(cuda) for g in grads]
    inv = hip.inverse_index(idx_d, n_pix)
    want_inv = torch.full((n_pix,), -1, dtype=torch.int32)
    want_inv[idx] = torch.arange(ns, dtype=torch.int32)
    assert torch.equal(inv.cpu(), want_inv)
    dense = hip.scatter_rows(specs, rows_on_device(rows, cuda), inv, n_pix, ns)
    for k, (d, want) in enumerate(zip(dense, ec.scatter_dense(specs, rows, idx, n_pix))):
        assert torch.equal(d.cpu(), want), 'scatter output %d %s' % (k, specs[k])
    for k, (g, want) in enumerate(zip(hip.gather_rows(specs, grads_d, idx_d, n_pix, ns), ec.gather_dense(specs, grads, idx))):
        assert torch.equal(g.cpu(), want), 'gather output %d %s' % (k, specs[k])
    for k, (g, want) in enumerate(zip(hip.gather_rows(specs, grads_d, idx_d, n_pix, ns, inv=inv), ec.gather_dense(specs, grads, idx))):
        assert torch.equal(g.cpu(), want), 'gather (valid, nothing padded) output %d %s' % (k, specs[k])


@pytest.mark.parametrize('shape', ec.SCATTER_SHAPES, ids=ec.scatter_id)
def test_gather_rows_on_a_padded_index_list(cuda, shape):
    """hip.surface_index at a capacity above the live count repeats the last pixel; hip.inverse_index maps it to its FIRST row: the
    rows behind receive exact zeros in the gather and are dropped by the scatter."""
    from psnerf_amd import hip
    n_pix, ns = shape
    specs = list(ec.SCATTER_SPECS)
    idx, _, grads = ec.scatter_inputs(n_pix, ns)
    cap = ns + 5
    mask = torch.zeros(n_pix, dtype=torch.bool)
    mask[idx] = True
    idx_p, count = hip.surface_index(mask.to(cuda), cap)
    assert float(count) == ns and torch.equal(idx_p.cpu(), torch.cat([idx, idx[-1:].expand(cap - ns)]))
    inv = hip.inverse_index(idx_p, n_pix, count)
    want_inv = torch.full((n_pix,), -1, dtype=torch.int32)
    want_inv[idx] = torch.arange(ns, dtype=torch.int32)
    assert torch.equal(inv.cpu(), want_inv)
    live = torch.arange(cap) < ns
    got = hip.gather_rows(specs, [g.to(cuda) for g in grads], idx_p, n_pix, cap, inv=inv)
    for k, (g, want) in enumerate(zip(got, ec.gather_dense(specs, grads, idx_p.cpu(), live=live))):
        assert torch.equal(g.cpu(), want), 'gather output %d %s' % (k, specs[k])
        assert not g.view(specs[k][0], cap, specs[k][1])[:, ns:].any()
    gen = torch.Generator().manual_seed(n_pix + ns)
    rows_p = [torch.randn(B * cap, C, generator=gen) for B, C, _ in specs]
    dense = hip.scatter_rows(specs, [r.to(cuda) for r in rows_p], inv, n_pix, cap)
    live_rows = [r.view(B, cap, C)[:, :ns].reshape(B * ns, C) for (B, C, _), r in zip(specs, rows_p)]
    for k, (d, want) in enumerate(zip(dense, ec.scatter_dense(specs, live_rows, idx, n_pix))):
        assert torch.equal(d.cpu(), want), 'scatter output %d %s' % (k, specs[k])


@pytest.mark.parametrize('padded', [False, True])
def test_scatter_rows_under_autograd(cuda, padded):
    """One output left without a gradient: its input gets None, the others the gathered rows (zeros on the dead rows of a padded list)."""
    from psnerf_amd import hip, ops
    n_pix, ns = 37, 12
    specs = tuple(ec.SCATTER_SPECS[:4])
    idx, rows, grads = ec.scatter_inputs(n_pix, ns, specs=ec.SCATTER_SPECS[:4])
    n_rows, live = ns, None
    if padded:
        n_rows = ns + 4
        mask = torch.zeros(n_pix, dtype=torch.bool)
        mask[idx] = True
        idx_d, count = hip.surface_index(mask.to(cuda), n_rows)
        inv = hip.inverse_index(idx_d, n_pix, count)
        live = torch.arange(n_rows) < ns
        gen = torch.Generator().manual_seed(99)
        rows = [torch.randn(B * n_rows, C, generator=gen) for B, C, _ in specs]
    else:
        idx_d = idx.to(cuda)
        inv = hip.inverse_index(idx_d, n_pix)
    leaf = [r.contiguous().to(cuda).requires_grad_() for r in rows]
    dense = ops.ScatterRows.apply(idx_d, inv, specs, *leaf)
    unused = 2
    sum((d * g.to(cuda)).sum() for k, (d, g) in enumerate(zip(dense, grads)) if k != unused).backward()
    want = ec.gather_dense(specs, grads, idx_d.cpu(), live=live)
    for k in range(len(specs)):
        if k == unused:
            assert leaf[k].grad is None
        else:
            assert torch.equal(leaf[k].grad.cpu(), want[k]), 'row gradient %d' % k
