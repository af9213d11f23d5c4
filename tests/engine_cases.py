"""Inputs and the float64 definitions for the direct tests of the three fused autograd engines (ops.VisibilityPair, ops.AppNetFused,
ops.GeoFieldFused) and of the two kernels under them that had no test of their own (psn_pe_encode_jvp; psn_scatter_rows /
psn_gather_rows / psn_gather_rows_valid).  Every definition is plain torch with autograd doing the differentiation, evaluated in
float64 ("truth") and in float32 on the CPU ("the reference arithmetic") from the same float32 inputs and weights.  Plain data and
reference code: nothing here touches a GPU.  The encoded input tables of the two ReLU engines are INPUTS of a case (the engines
take them as such): the GPU tests hand in what hip.pe_encode / hip.app_input wrote, the CPU tests the torch statement below.

ReLU kinks.  A hidden unit whose pre-activation is within rounding of zero may be on in one float32 evaluation and off in another;
its whole incoming gradient then moves, which is no error of either.  Decided by the reference alone, per case:
    eps  = 4 x max |z_fp32(CPU) - z_float64| over all hidden pre-activations (an independent rounding of the same sums; the factor
           covers a second summation order plus the propagated error of the layers below),
    rows with any hidden |z_float64| <= eps receive ZERO upstream gradient -- in the device run and in both reference runs, so they
    contribute to no compared tensor.  KINK_CAP: at most 5 % of a case's rows (tests/test_engines_cpu.py asserts it).
The geometry field is softplus and needs none of this."""
import numpy as np
import torch

from oracle import stage1 as o1
from oracle import stage2 as o2
from tests.helpers import stage1_cfg, stage1_state_dict, stage2_state_dict

KINK_CAP = 0.05
PE_STRIDE = 64


def _f64(t):
    return t.detach().double().cpu().numpy()


# --------------------------------------------------------------------------- encodings
def encode(x, n_freqs, scale=1.0):
    """[x s, sin(2^k x s), cos(2^k x s)]_{k < n_freqs} in the dtype of x (oracle.stage1.positional_encoding = oracle.stage2.embed)."""
    xs = x * scale
    return torch.cat([xs] + [f(xs * float(2 ** k)) for k in range(n_freqs) for f in (torch.sin, torch.cos)], -1)


def pe_table(x, n_freqs, scale=1.0, stride=PE_STRIDE):
    """The table hip.pe_encode writes, stated in torch: the encoding in the leading 3 + 6 n_freqs columns, zeros up to ``stride``."""
    pe = encode(x, n_freqs, scale)
    return torch.nn.functional.pad(pe, (0, stride - pe.shape[1])).contiguous()


def pe_jvp(x, t, n_freqs, scale=1.0, stride=PE_STRIDE, dtype=torch.float64):
    """J_encode(x) t by torch.autograd.functional.jvp in ``dtype``, laid out as hip.pe_encode_jvp lays it out: [n, stride] whose
    PADDING columns 3 + 6 n_freqs .. stride are exact zeros (ops.GeoFieldFused.backward feeds the whole 64-column table to a chain
    launch as its input-feature k-tiles: anything else there would be multiplied into d a_0)."""
    jv = torch.autograd.functional.jvp(lambda y: encode(y, n_freqs, scale), x.to(dtype), t.to(dtype))[1]
    return torch.nn.functional.pad(jv, (0, stride - jv.shape[1]))


PE_JVP_CASES = [(n, f, s) for n in (1, 63, 1000) for f in (0, 6, 10) for s in (1.0, 0.5)]


def pe_jvp_inputs(n, n_freqs, scale):
    g = torch.Generator().manual_seed(7000 + 13 * n + n_freqs)
    return torch.rand(n, 3, generator=g) * 2.4 - 1.2, torch.randn(n, 3, generator=g)


# --------------------------------------------------------------------------- ReLU MLP + kink analysis
def relu_mlp(inp, Ws, bs, skip_at=None):
    """oracle.stage2.MLP (final = 'linear'): the skip concatenates the INPUT behind the output of layer ``skip_at``.
    -> (output, [pre-activation z_l of every hidden layer])."""
    h, zs, n = inp, [], len(Ws)
    for l in range(n):
        z = h @ Ws[l].t() + bs[l]
        if l == n - 1:
            return z, zs
        zs.append(z)
        h = torch.relu(z)
        if l == skip_at:
            h = torch.cat([h, inp], -1)


def kink_rows(forward):
    """forward(dtype) -> list of hidden pre-activations [rows, width].  -> (eps, bool [rows]: any hidden |z_float64| <= eps)."""
    with torch.no_grad():
        z64, z32 = forward(torch.float64), forward(torch.float32)
    eps = 4.0 * max(float((a.double() - b).abs().max()) for a, b in zip(z32, z64))
    near = torch.zeros(z64[0].shape[0], dtype=torch.bool)
    for z in z64:
        near |= (z.abs() <= eps).any(-1)
    return eps, near


KINK_KEEP = 0.03


def take_points(n, rows_near, rows_per_point):
    """Indices of the first ``n`` candidate points in drawn order, of which those with rows near a kink (rows_near [M] counts) are
    taken only while such rows stay within KINK_KEEP of the case's n * rows_per_point rows: the masking is exercised, the cap kept."""
    budget, keep = int(KINK_KEEP * n * rows_per_point), []
    for i, bad in enumerate(rows_near.tolist()):
        if len(keep) == n:
            break
        if bad <= budget:
            budget -= bad
            keep.append(i)
    assert len(keep) == n, '%d of %d candidate points taken' % (len(keep), rows_near.numel())
    return torch.tensor(keep, dtype=torch.long)


def _leaves(ts, dtype):
    return [t.detach().to(dtype).clone().requires_grad_(True) for t in ts]


def _param_grads(res, Ws, bs):
    for l, (W, b) in enumerate(zip(Ws, bs)):
        res['dW%d' % l], res['db%d' % l] = _f64(W.grad), _f64(b.grad)


# --------------------------------------------------------------------------- visibility net (ops.VisibilityPair)
VIS_FREQS, VIS_DIN_HALF, VIS_SKIP_AT = 10, 63, 4
# (Ns, L, V): one row | a partial tile | the dump window starts on a 64-row boundary but not a 128-row one | ragged on both sides |
# save_row0 = 666: the supervised rows begin mid-tile | the V <= 16 grouped pair_sums path at its limit | the V > 16 path
VIS_CASES = [(1, 1, 1), (63, 1, 2), (64, 2, 1), (130, 1, 3), (333, 2, 3), (128, 3, 16), (96, 1, 17)]
_VIS_W = []


def vis_id(spec):
    return 'Ns%d-L%d-V%d' % spec


def vis_weights():
    """(Ws, bs) of the shipped visibility net: 9 linears, width 256, skip_at 4, 2 x 63 inputs (helpers.stage2_state_dict, seed 31)."""
    if not _VIS_W:
        sd = stage2_state_dict(o2.bear_conf(), seed=31)
        n = len([k for k in sd if k.startswith('visibility_net.linears.') and k.endswith('.weight')])
        _VIS_W.extend([[sd['visibility_net.linears.%d.%s' % (l, kind)].float().contiguous() for l in range(n)] for kind in ('weight', 'bias')])
        assert n == 9 and _VIS_W[0][0].shape == (256, 2 * VIS_DIN_HALF) and _VIS_W[0][VIS_SKIP_AT + 1].shape == (256, 256 + 2 * VIS_DIN_HALF)
    return _VIS_W


_VIS_PTS = {}


def vis_points(spec):
    """Surface points [Ns,3] and unit light directions [L+V,3], drawn as test_fused_visibility_mlp draws them -- the points by
    rejection: of 4 Ns (12 Ns for V > 3) candidates the first Ns, a candidate any of whose V supervised rows has a hidden float64
    pre-activation within the candidates' own margin of zero (kink_rows; the reference alone decides) being taken only while such rows
    stay within 3 % of the case (take_points).  Drawn without it, 5.7 - 8.0 % of the rows of
    the cases below are masked at eps = 2.9 - 4.3e-6 -- over the cap: the 126-term sums of layer 0 run through partial sums of up to 2
    and differ by 9e-7 between float32 and float64 in ANY summation order, while the deep layers (rms z = 0.04) put 256 units per
    row and layer close to zero.  The cap is asserted on the case as it stands, with the case's own eps."""
    if spec not in _VIS_PTS:
        Ns, L, V = spec
        g = torch.Generator().manual_seed(800 + Ns + 7 * L + 31 * V)
        M = Ns * (4 if V <= 3 else 12)
        x = torch.rand(M, 3, generator=g) * 1.2 - 0.6
        l = torch.nn.functional.normalize(torch.randn(L + V, 3, generator=g), dim=-1)
        Ws, bs = vis_weights()
        rows = vis_rows(pe_table(x, VIS_FREQS), pe_table(l[L:], VIS_FREQS))
        _, near = kink_rows(lambda dt: relu_mlp(rows.to(dt), [w.to(dt) for w in Ws], [b.to(dt) for b in bs], VIS_SKIP_AT)[1])
        keep = take_points(Ns, near.view(V, M).sum(0), V)
        _VIS_PTS[spec] = (x[keep].contiguous(), l)
    return _VIS_PTS[spec]


def vis_rows(pe_x, pe_l):
    """The expanded input block, light-major: row k = [PE(x)[k % Ns] | PE(l)[k // Ns]]."""
    Ns, LV, d = pe_x.shape[0], pe_l.shape[0], VIS_DIN_HALF
    return torch.cat([pe_x[:, :d].tile(LV, 1), pe_l[:, :d].repeat_interleave(Ns, dim=0)], -1)


def vis_case(spec, pe_x=None, pe_l=None):
    """The complete case on the float32 tables pe_x [Ns,64] / pe_l [L+V,64] (default: pe_table of vis_points): 'c' [V*Ns,1] = the
    seeded upstream gradient of vis_t, ZERO on the 'masked' rows; 'eps', 'share' = the masked share of the supervised rows."""
    Ns, L, V = spec
    x, l = vis_points(spec)
    pe_x = pe_table(x, VIS_FREQS) if pe_x is None else pe_x.detach().cpu().float()
    pe_l = pe_table(l, VIS_FREQS) if pe_l is None else pe_l.detach().cpu().float()
    assert pe_x.shape == (Ns, PE_STRIDE) and pe_l.shape == (L + V, PE_STRIDE)
    Ws, bs = vis_weights()
    rows = vis_rows(pe_x, pe_l)
    eps, near = kink_rows(lambda dt: relu_mlp(rows.to(dt), [w.to(dt) for w in Ws], [b.to(dt) for b in bs], VIS_SKIP_AT)[1])
    masked = near[L * Ns:]
    c = torch.randn(V * Ns, 1, generator=torch.Generator().manual_seed(900 + Ns)) * (~masked).float()[:, None]
    return dict(spec=spec, x=x, l=l, pe_x=pe_x, pe_l=pe_l, c=c, eps=eps, masked=masked, share=float(masked.float().mean()), refs={})


def vis_reference(case, dtype):
    """-> float64 ndarrays: vis [L*Ns,1], vis_t [V*Ns,1] and dW_l / db_l of (vis_t * c).sum(), evaluated in ``dtype``."""
    if dtype not in case['refs']:
        Ns, L, V = case['spec']
        Ws, bs = (_leaves(t, dtype) for t in vis_weights())
        out, _ = relu_mlp(vis_rows(case['pe_x'], case['pe_l']).to(dtype), Ws, bs, VIS_SKIP_AT)
        (out[L * Ns:] * case['c'].to(dtype)).sum().backward()
        res = {'vis': _f64(out[:L * Ns]), 'vis_t': _f64(out[L * Ns:])}
        _param_grads(res, Ws, bs)
        case['refs'][dtype] = res
    return case['refs'][dtype]


# --------------------------------------------------------------------------- appearance net (ops.AppNetFused)
# Q at the shipped d_x = 3 + d_view + 3 = 33; 'full': a network whose d_x = 64 fills whole k-tiles (the d normal columns are the last
# of a tile), random weights of the right shapes
APP_CASES = [(1, 'bear'), (63, 'bear'), (64, 'bear'), (65, 'bear'), (130, 'bear'), (1000, 'bear'), (130, 'full')]
_APP_W = {}


def app_id(spec):
    return 'Q%d-%s' % spec


def _stage1_net():
    cfg = stage1_cfg('bear')
    net = o1.NeuralNetwork(cfg)
    net.load_state_dict(stage1_state_dict(cfg, seed=21))
    return net


def app_weights(kind):
    """(Ws, bs, d_x, n_freqs of the view encoding).  'bear': the effective matrices w = v (g / |v|_row) of the stage-1 BEAR
    appearance layers -- the expression NeuralNetwork._app_params evaluates on the host (test_engines_cpu.py asserts the identity)."""
    if kind not in _APP_W:
        if kind == 'bear':
            net = _stage1_net()
            with torch.no_grad():
                Ws = [getattr(net, 'lina%d' % l).weight().float().contiguous() for l in range(net.n_app)]
                bs = [getattr(net, 'lina%d' % l).bias.detach().float().clone() for l in range(net.n_app)]
            _APP_W[kind] = (Ws, bs, 3 + (3 + 6 * net.octaves_pe_views) + 3, net.octaves_pe_views)
        else:
            g = torch.Generator().manual_seed(4100)
            dims = [(256, 64 + 256)] + [(256, 256)] * 3 + [(3, 256)]
            _APP_W[kind] = ([torch.randn(o, i, generator=g) * (1.2 / i ** 0.5) for o, i in dims],
                            [torch.randn(o, generator=g) * 0.05 for o, _ in dims], 64, None)
    return _APP_W[kind]


_APP_PTS = {}


def _app_draw(Q, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(Q, 3, generator=g) * 1.6 - 0.8
    v = torch.randn(Q, 3, generator=g) * (0.5 + torch.rand(Q, 1, generator=g))
    nrm = torch.nn.functional.normalize(torch.randn(Q, 3, generator=g), dim=-1) * (0.8 + 0.4 * torch.rand(Q, 1, generator=g))
    return p, v, nrm, torch.randn(Q, 256, generator=g) * 0.5


def _app_rows(kind, p, v, nrm, seed):
    """[M,64]: [p | gamma(v / |v|) | normal | 0]; 'full': 64 seeded columns."""
    if kind == 'full':
        return torch.rand(p.shape[0], 64, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0
    x = torch.cat([p, encode(v / torch.norm(v, dim=-1, keepdim=True), app_weights(kind)[3]), nrm], -1)
    return torch.nn.functional.pad(x, (0, PE_STRIDE - x.shape[1])).contiguous()


def app_points(spec):
    """points, raw view directions, normals [Q,3], geometry features [Q,256] and the CPU statement of the [Q,64] input table: of
    2 Q + 8 seeded candidates the first Q, rows near a kink by the candidates' own margin up to 3 % of the case (as vis_points; drawn
    without it, up to 6.2 % of a case's rows are masked at eps = 2.8 - 6.0e-6)."""
    if spec not in _APP_PTS:
        Q, kind = spec
        Ws, bs, d_x, _ = app_weights(kind)
        p, v, nrm, feat = _app_draw(2 * Q + 8, 4000 + Q)
        x = _app_rows(kind, p, v, nrm, 4200 + Q)
        _, near = kink_rows(lambda dt: app_forward(x[:, :d_x - 3].to(dt), x[:, d_x - 3:d_x].to(dt), feat.to(dt), [w.to(dt) for w in Ws],
                                                   [b.to(dt) for b in bs])[1])
        keep = take_points(Q, near.long(), 1)
        _APP_PTS[spec] = tuple(t[keep].contiguous() for t in (p, v, nrm, feat, x))
    return _APP_PTS[spec]


def app_table(spec):
    """The table hip.app_input writes for app_points(spec), stated in torch ('full': the seeded 64-column table itself)."""
    return app_points(spec)[4]


def app_forward(x, normal, feat, Ws, bs):
    """stage-1 infer_app before its tanh: the ReLU MLP on cat[x[:, :d_x - 3], normal, feat] -> (pre-activation colour [Q,3], zs)."""
    return relu_mlp(torch.cat([x, normal, feat], -1), Ws, bs)


def app_case(spec, x=None):
    """The complete case on the float32 input table x [Q,64] (default: app_table): 'normal' = its columns d_x - 3 .. d_x, 'feat',
    'c' [Q,3] = the seeded upstream gradient, ZERO on the 'masked' rows; 'eps', 'share'."""
    Q, kind = spec
    Ws, bs, d_x, _ = app_weights(kind)
    x = app_table(spec) if x is None else x.detach().cpu().float()
    assert x.shape == (Q, PE_STRIDE)
    feat = app_points(spec)[3]
    normal = x[:, d_x - 3:d_x].contiguous()
    eps, masked = kink_rows(lambda dt: app_forward(x[:, :d_x - 3].to(dt), normal.to(dt), feat.to(dt), [w.to(dt) for w in Ws],
                                                   [b.to(dt) for b in bs])[1])
    c = torch.randn(Q, 3, generator=torch.Generator().manual_seed(4300 + Q)) * (~masked).float()[:, None]
    return dict(spec=spec, x=x, normal=normal, feat=feat, d_x=d_x, c=c, eps=eps, masked=masked, share=float(masked.float().mean()), refs={})


def app_reference(case, dtype):
    """-> float64 ndarrays: y [Q,3], d_normal (the gradient of the normal columns ALONE), d_feat, dW_l / db_l of (y * c).sum()."""
    if dtype not in case['refs']:
        Ws, bs = (_leaves(t, dtype) for t in app_weights(case['spec'][1])[:2])
        normal, feat = _leaves([case['normal'], case['feat']], dtype)
        y, _ = app_forward(case['x'][:, :case['d_x'] - 3].to(dtype), normal, feat, Ws, bs)
        (y * case['c'].to(dtype)).sum().backward()
        res = {'y': _f64(y), 'd_normal': _f64(normal.grad), 'd_feat': _f64(feat.grad)}
        _param_grads(res, Ws, bs)
        case['refs'][dtype] = res
    return case['refs'][dtype]


# --------------------------------------------------------------------------- geometry field (ops.GeoFieldFused)
def geo_field(pts, params, octaves, skips, scale):
    """The stage-1 geometry network on points ``pts`` (a leaf that requires a gradient) with the EFFECTIVE parameters ``params`` =
    [W0, b0, W1, b1, ...] (the 1 / sqrt(2) of the skip layer folded in): encoding, softplus-100 layers, skip connection, and
    d logit / d p by autograd.grad(create_graph=True).  In the dtype and on the device of its arguments.
    -> (logit [Q,1], feat [Q,256], grad [Q,3])."""
    pe = encode(pts, octaves, scale)
    h = pe
    n = len(params) // 2
    for l in range(n):
        if l in skips:
            h = torch.cat([h, pe], -1)
        h = h @ params[2 * l].t() + params[2 * l + 1]
        if l < n - 1:
            h = torch.nn.functional.softplus(h, beta=100)
    grad = torch.autograd.grad(h[:, :1].sum(), pts, create_graph=True)[0]
    return h[:, :1], h[:, 1:], grad


_GEO_W = []


def geo_weights():
    """(params [W0, b0, ...] effective with the skip layer's 1 / sqrt(2) folded in as NeuralNetwork._geo_params folds it on the host,
    octaves, skips, scale) of the geometric-init BEAR network (helpers.stage1_state_dict, seed 21)."""
    if not _GEO_W:
        net = _stage1_net()
        inv = float(1.0 / np.sqrt(2))
        params = []
        with torch.no_grad():
            for l in range(net.n_geo):
                lin = getattr(net, 'lin%d' % l)
                params += [(lin.weight() * inv if l in net.skips else lin.weight()).float().contiguous(), lin.bias.detach().float().clone()]
        _GEO_W.extend([params, net.octaves_pe, tuple(net.skips), 1.0 / net.rescale])
    return _GEO_W


# Q, feat_rows (None = Q), with_grad, the outputs the objective uses
_ALL = ('logit', 'feat', 'grad')
GEO_CASES = ([dict(Q=q, feat_rows=None, with_grad=True, use=_ALL) for q in (1, 65, 130, 1000)]
             + [dict(Q=1000, feat_rows=r, with_grad=True, use=_ALL) for r in (1, 63, 64, 999)]
             + [dict(Q=130, feat_rows=None, with_grad=False, use=('logit', 'feat')), dict(Q=1000, feat_rows=63, with_grad=False, use=('logit', 'feat'))]
             + [dict(Q=130, feat_rows=None, with_grad=True, use=tuple(k for k in _ALL if k != drop)) for drop in _ALL])


def geo_id(spec):
    return 'Q%d-feat%s-%s-%s' % (spec['Q'], spec['feat_rows'], 'grad' if spec['with_grad'] else 'nograd', '+'.join(spec['use']))


_GEO = {}


def geo_case(spec):
    """points and the seeded weights of the linear objective (logit * c_logit + feat[:feat_rows] * c_feat + grad * c_grad).sum()
    restricted to spec['use'].  Cached; treat as read-only."""
    key = geo_id(spec)
    if key not in _GEO:
        Q, fr = spec['Q'], spec['feat_rows'] or spec['Q']
        g = torch.Generator().manual_seed(5000 + Q + fr)
        _GEO[key] = dict(spec=spec, pts=(torch.rand(Q, 3, generator=g) - 0.5) * 1.6, c_logit=torch.randn(Q, 1, generator=g),
                         c_feat=torch.randn(fr, 256, generator=g) * 0.1, c_grad=torch.randn(Q, 3, generator=g), feat_rows=fr, refs={})
    return _GEO[key]


def geo_objective(case, logit, feat, grad):
    """``feat`` = the first feat_rows rows.  The same expression for the engine's outputs and the definition's."""
    use, dt, dev = case['spec']['use'], logit.dtype, logit.device
    terms = []
    if 'logit' in use:
        terms.append((logit * case['c_logit'].to(dev, dt)).sum())
    if 'feat' in use:
        terms.append((feat * case['c_feat'].to(dev, dt)).sum())
    if 'grad' in use:
        terms.append((grad * case['c_grad'].to(dev, dt)).sum())
    return sum(terms)


def geo_reference(case, dtype):
    """-> float64 ndarrays: logit [Q,1], feat [feat_rows,256], grad [Q,3] and dW_l / db_l of geo_objective (a parameter the
    objective does not reach has a zero gradient)."""
    if dtype not in case['refs']:
        params, octaves, skips, scale = geo_weights()
        P = _leaves(params, dtype)
        logit, feat, grad = geo_field(case['pts'].to(dtype).requires_grad_(True), P, octaves, skips, scale)
        feat = feat[:case['feat_rows']]
        geo_objective(case, logit, feat, grad).backward()
        res = {'logit': _f64(logit), 'feat': _f64(feat), 'grad': _f64(grad)}
        for l in range(len(P) // 2):
            for name, p in (('dW%d' % l, P[2 * l]), ('db%d' % l, P[2 * l + 1])):
                res[name] = _f64(torch.zeros_like(p) if p.grad is None else p.grad)
        case['refs'][dtype] = res
    return case['refs'][dtype]


# --------------------------------------------------------------------------- scatter_rows / gather_rows (ops.ScatterRows)
SCATTER_SHAPES = [(1, 1), (37, 1), (37, 37), (37, 12), (4099, 1), (4099, 4099), (4099, 1366)]   # (N pixels, Ns surface rows)
# 17 outputs in one call (one more than SCATTER_MAX_ITEMS = a second launch): B in {1, 3}, C in {1, 3, 9}, fills 0, 1 and -2.5
SCATTER_SPECS = [((1, 3)[i % 2], (1, 3, 9)[i % 3], (0.0, 1.0, -2.5)[(i // 2) % 3]) for i in range(17)]
SCATTER_EXPAND, SCATTER_SLICE = 1, 4   # rows with a stride-0 column (expand of [B*Ns,1]) / a non-contiguous column slice of a wider tensor


def scatter_id(shape):
    return 'N%d-Ns%d' % shape


def scatter_inputs(n_pix, ns, specs=SCATTER_SPECS):
    """idx [Ns] int64 ascending pixel positions, rows (a list of [B*Ns, C] float32 tensors, two of them strided views), dense gradients."""
    g = torch.Generator().manual_seed(6000 + n_pix + ns)
    idx = torch.randperm(n_pix, generator=g)[:ns].sort().values
    rows = []
    for i, (B, C, _) in enumerate(specs):
        if i == SCATTER_EXPAND:
            assert C > 1
            rows.append(torch.randn(B * ns, 1, generator=g).expand(B * ns, C))
        elif i == SCATTER_SLICE:
            rows.append(torch.randn(B * ns, C + 3, generator=g)[:, 1:1 + C])
        else:
            rows.append(torch.randn(B * ns, C, generator=g))
    assert len(specs) < 17 or (rows[SCATTER_EXPAND].stride(1) == 0 and rows[SCATTER_SLICE].stride(0) == specs[SCATTER_SLICE][1] + 3)
    return idx, rows, [torch.randn(B, n_pix, C, generator=g) for B, C, _ in specs]


def scatter_dense(specs, rows, idx, n_pix):
    """dense_k [B, N, C] = fill_k, dense_k[:, idx] = rows_k (light-major rows)."""
    out = []
    for (B, C, fill), r in zip(specs, rows):
        d = torch.full((B, n_pix, C), float(fill), dtype=torch.float32)
        d[:, idx] = r.reshape(B, idx.numel(), C)
        out.append(d)
    return out


def gather_dense(specs, grads, idx, live=None):
    """The adjoint: grad_k[:, idx] as [B*Ns, C]; ``live`` (bool [Ns]): the other rows of a padded index list are exact zeros."""
    out = []
    for (B, C, _), g in zip(specs, grads):
        r = g[:, idx]
        if live is not None:
            r = torch.where(live[None, :, None], r, torch.zeros_like(r))
        out.append(r.reshape(B * idx.numel(), C))
    return out
