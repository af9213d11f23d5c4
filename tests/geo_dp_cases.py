"""Cases and float64 definitions for the point gradient of the stage-1 geometry field: the contract of psn_geo_point_grad stated in
numpy (any float dtype: float64 = truth, float32 = the reference arithmetic), the geometry field of tests/engine_cases.py restated
with its intermediates exposed (for the derivation check of tests/test_geo_dp_cpu.py), and geo_reference extended by pts.grad.
Plain data and reference code: nothing here touches a GPU.  engine_cases is imported read-only (its caches are not written to)."""
import numpy as np
import torch

from tests import engine_cases as ec


# --------------------------------------------------------------------------- the kernel's contract
def encoding_columns(n_freqs):
    """Per encoding column k: (coordinate c, octave f or -1 for the identity, is_cos)."""
    cols = [(c, -1, False) for c in range(3)]
    for f in range(n_freqs):
        cols += [(c, f, False) for c in range(3)] + [(c, f, True) for c in range(3)]
    return cols


def point_grad_contract(p, n_freqs, scale, dz0, w0, dzs=None, ws=None, g_pe=None, g_pe2=None, d_grad=None, dtype=np.float64):
    """psn_geo_point_grad in numpy, every operand converted to ``dtype`` first:
        t = dz0 w0[:, :d_pe] (+ dzs ws[:, :d_pe]);  d_p[:, c] = sum_k J_k t_k (+ d_grad[:, c] sum_k H_k (g_pe + g_pe2)_k)
    over the columns k of coordinate c, J = s | 2^f s cos | -2^f s sin, H = 0 | -(2^f s)^2 sin | -(2^f s)^2 cos at 2^f s p_c."""
    cv = lambda t: None if t is None else np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).astype(dtype)
    p, dz0, w0, dzs, ws, g_pe, g_pe2, d_grad = (cv(t) for t in (p, dz0, w0, dzs, ws, g_pe, g_pe2, d_grad))
    d_pe, s = 3 + 6 * n_freqs, dtype(scale)
    t = dz0 @ w0[:, :d_pe]
    if dzs is not None:
        t = t + dzs @ ws[:, :d_pe]
    g = None
    if g_pe is not None:
        g = g_pe[:, :d_pe] if g_pe2 is None else g_pe[:, :d_pe] + g_pe2[:, :d_pe]
    out = np.zeros((p.shape[0], 3), dtype=dtype)
    hess = np.zeros((p.shape[0], 3), dtype=dtype)
    for k, (c, f, is_cos) in enumerate(encoding_columns(n_freqs)):
        if f < 0:
            out[:, c] += s * t[:, k]
            continue
        a = dtype(2.0 ** f) * s
        arg = a * p[:, c]
        out[:, c] += (-a * np.sin(arg) if is_cos else a * np.cos(arg)) * t[:, k]
        if g is not None:
            hess[:, c] += -(a * a) * (np.cos(arg) if is_cos else np.sin(arg)) * g[:, k]
    return out if g is None else out + d_grad * hess


KERNEL_ROWS = (1, 63, 64, 65, 130, 1000)
KERNEL_ENCODINGS = ((6, 1.0), (6, 0.5), (10, 1.0), (0, 1.0))
# (h0, hs): the shipped shape | no skip block | widths that are no multiple of the k-step | one column | a stacked block beyond
# the LDS budget at n_freqs = 10 (staged in k-chunks per row tile)
KERNEL_WIDTHS = ((256, 256), (256, None), (64, 40), (1, None), (512, 512))
KERNEL_SECOND = ('none', 'one', 'two')   # no second-order group | g_pe alone (g_pe2 NULL) | g_pe and g_pe2
PAD = 5                                   # every matrix operand is a column range [PAD : PAD + width] of a wider tensor


def kernel_inputs(n, n_freqs, h0, hs, second):
    """Seeded float32 operands of one kernel case, each matrix WIDER than its operand (the caller slices [:, PAD:PAD + width])."""
    g = torch.Generator().manual_seed(9000 + 7 * n + 131 * n_freqs + h0 + 3 * (hs or 0))
    d_pe = 3 + 6 * n_freqs
    rnd = lambda r, c, s=1.0: torch.randn(r, c + 2 * PAD, generator=g) * s
    out = dict(p=torch.rand(n, 3, generator=g) * 2.4 - 1.2, dz0=rnd(n, h0), w0=rnd(h0, d_pe, h0 ** -0.5))
    if hs is not None:
        out.update(dzs=rnd(n, hs), ws=rnd(hs, d_pe, hs ** -0.5))
    if second != 'none':
        out.update(g_pe=rnd(n, d_pe), d_grad=torch.randn(n, 3, generator=g))
        if second == 'two':
            out['g_pe2'] = rnd(n, d_pe)
    return out


def kernel_views(inp, n_freqs):
    """The operand views of kernel_inputs (row stride > width) as keyword arguments of hip.geo_point_grad / point_grad_contract."""
    d_pe = 3 + 6 * n_freqs
    kw = {}
    for k, t in inp.items():
        if k in ('p', 'd_grad'):
            kw[k] = t
        else:
            kw[k] = t[:, PAD:PAD + (d_pe if k in ('w0', 'ws', 'g_pe', 'g_pe2') else t.shape[1] - 2 * PAD)]
    return kw


# --------------------------------------------------------------------------- the field with its intermediates
def geo_field_parts(pts, params, octaves, skips, scale):
    """engine_cases.geo_field operation for operation, returning also the encoding and the pre-activations:
    -> (logit, feat, grad, pe, [z_l])."""
    pe = ec.encode(pts, octaves, scale)
    h, zs = pe, []
    n = len(params) // 2
    for l in range(n):
        if l in skips:
            h = torch.cat([h, pe], -1)
        h = h @ params[2 * l].t() + params[2 * l + 1]
        zs.append(h)
        if l < n - 1:
            h = torch.nn.functional.softplus(h, beta=100)
    grad = torch.autograd.grad(h[:, :1].sum(), pts, create_graph=True)[0]
    return h[:, :1], h[:, 1:], grad, pe, zs


# --------------------------------------------------------------------------- geo_reference + d_p
_REFS = {}


def geo_reference_dp(case, dtype):
    """engine_cases.geo_reference (same expressions, same leaves) extended by 'd_p' = pts.grad of geo_objective [Q,3].  Cached here."""
    key = (ec.geo_id(case['spec']), dtype)
    if key not in _REFS:
        params, octaves, skips, scale = ec.geo_weights()
        P = ec._leaves(params, dtype)
        pts = case['pts'].detach().clone().to(dtype).requires_grad_(True)   # (the cached tensor itself stays as it is)
        logit, feat, grad = ec.geo_field(pts, P, octaves, skips, scale)
        feat = feat[:case['feat_rows']]
        ec.geo_objective(case, logit, feat, grad).backward()
        res = {'logit': ec._f64(logit), 'feat': ec._f64(feat), 'grad': ec._f64(grad), 'd_p': ec._f64(pts.grad)}
        for l in range(len(P) // 2):
            for name, q in (('dW%d' % l, P[2 * l]), ('db%d' % l, P[2 * l + 1])):
                res[name] = ec._f64(torch.zeros_like(q) if q.grad is None else q.grad)
        _REFS[key] = res
    return _REFS[key]


GEOFIELD_CASES = [dict(Q=65, feat_rows=None, with_grad=True, use=ec._ALL), dict(Q=1000, feat_rows=None, with_grad=True, use=ec._ALL),
                  dict(Q=65, feat_rows=None, with_grad=False, use=('logit', 'feat'))]
