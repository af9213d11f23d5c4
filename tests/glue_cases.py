"""Cases, float64 truths and float32 restatements for the kernels that run AROUND the fused engines: csrc/pe.hip (encode, JVP,
backward, appearance input table), csrc/weight_norm.hip, the row / index / copy kernels of csrc/small.hip and csrc/views.hip.
Importable without a GPU: tests/test_glue_cpu.py checks the cases (paths reached, restatements within their caps, wrong
formulations rejected), tests/test_glue_gpu.py runs them on the device.  Every input comes from a seeded generator.

Per kernel: a TRUTH in float64; where the result is rounded, an fp32 RESTATEMENT of the reference formula in the kernel's
documented operation order; and a ``*_path(case)`` that names the launch path, recomputed from a copy of the entry point's
conditions.  The comparators (``check_*``) are shared by the GPU test (kernel output) and the CPU test (restatements, and
deliberately wrong formulations that must fail them).

Bounds (helpers.assert_vs_truth: elementwise |x - truth| <= rtol |truth| + atol; the kernel may have as many elements beyond
it as the restatement has beyond half of it and a worst element of max(1, 2 x the restatement's worst)):
    encodings, normalised rows, rays        RTOL_VALUE = 1e-6, atol ATOL_UNIT
    their gradients                         RTOL_GRAD  = 1e-5, atol = rtol x max|truth| (per tensor; per ROW for the normalize
                                            backward, whose rows span 30 orders of magnitude by construction)
    weight-norm forward / backward          2e-6 / 2e-5, atol = rtol x max|truth| of the item; for dv, rtol x max|dw g scale / |v||:
                                            dv is the difference of that term and its projection on v, each rounded relative
                                            to ITSELF, and the difference can vanish (it is exactly 0 for a one-column matrix)
Measured restatement figures are printed by test_glue_cpu.py; no bound had to be raised (worst restatement / bound: see there).

Conventions that make a truth well defined where fp32 has edges:
  * encodings: the truth is float64 sin / cos of the fp32-ROUNDED argument -- x * scale is rounded once, the 2^f scaling (ldexp)
    is exact -- so the only rounding under test is sinf / cosf.  The bands of the appearance table take the table's OWN view
    columns (v / |v| as the kernel rounded it, checked against float64 separately) as that argument.
  * normalize: a row whose squares overflow fp32 (components of 1e20; those of 1e18 still fit) has norm +inf BY the fp32
    formulation (torch's too) and normalises to exact zeros; the truth follows that definition, not the real-number value.
    Squares that fall into the denormals (1e-20) give an imprecise (or flushed) fp32 norm that is below eps like the float64 one:
    the same clamp branch, where the norm's value is not used, and the same value x / eps (one division: bit-equal).
  * weight norm, exact cases: rows of small integers whose sum of squares is a perfect square ((3, 4), (1, 2, 2), (2, 3, 6),
    spread over lanes and over columns >= 64), g and scale powers of two.  Every partial sum is an exact integer in any order, so
    |v| is exact and the forward v * (g / |v|) [* scale] is ONE sequence of correctly rounded operations without an addition
    (no fused multiply-add can form): bit-equal to its numpy restatement.  The backward's dot (integers) and dg = dot / |v| are
    exact in the same sense.  dv = dw * ss - k * v may be contracted to a fused multiply-add either way, so it is bit-equal only
    where the product k * v is exactly zero: elements with v = 0 and rows with dot = 0.  The other dv elements go through the
    bound.
  * weight norm, range of row norms: the fp32 torch formulation of nn.utils.weight_norm's backward (autograd of
    torch._weight_norm(v, g, 0)) divides by |v|^2; WN_TORCH_FINITE records the decades of |v| over which it stays finite AND
    within the backward bound of float64 on this module's inputs (measured by test_glue_cpu.py: 1e-19 .. 1e19; beyond, |v|^2
    leaves the fp32 range).  The kernel forms |v|^3 and is therefore narrower: WN_KERNEL_FINITE = 1e-13 .. 1e12 by the same
    measurement on its restatement (1e-13 only with denormal support: |v|^3 = 1e-39; above 1e12 the cube overflows and the
    projection term silently vanishes -- finite, but wrong).  Trained weight rows have norms of order 1; the kernel is tested at
    1e-6, 1 and 1e6, inside both ranges.
"""
import itertools

import numpy as np
import torch

from tests.helpers import ATOL_UNIT, assert_vs_truth

F32, F64 = np.float32, np.float64
RTOL_VALUE, RTOL_GRAD = 1e-6, 1e-5
RTOL_WN_FWD, RTOL_WN_BWD = 2e-6, 2e-5
GRID_CAP = 256 * 32            # blocks of 256 threads of the pe.hip entry points
PASS = GRID_CAP * 256          # work items of one pass of their grid-stride loops
BASE_ROWS = 1024               # the cap cases tile a base of this many rows
MAX_SHARE, MAX_WORST = 0.02, 4.0   # caps of an fp32 restatement (tests/test_ray_cpu.py)
WN_TORCH_FINITE = (1e-19, 1e19)
WN_KERNEL_FINITE = (1e-13, 1e12)
_WORST = {}                    # check name class -> (worst r_x, r_ref): filled by check(), printed by the tests
CAPS = False                   # set by tests/test_glue_cpu.py: check() also holds the restatement to MAX_SHARE / MAX_WORST
_CAPS = {}                     # check name class -> (worst share beyond half the bound, worst element / bound) of the restatement


def rng(*key):
    return np.random.default_rng([7] + [int(k) for k in key])


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32))


def check(name, got, ref, truth, rtol, atol, cls=None):
    """assert_vs_truth with NaN / inf patterns compared first (a special row must show the truth's pattern, and only it)."""
    g, r, t = (np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=F64) for a in (got, ref, truth))
    assert g.shape == t.shape == r.shape, '%s: shapes %s %s %s' % (name, g.shape, r.shape, t.shape)
    fin = np.isfinite(t)
    assert np.array_equal(np.isnan(g), np.isnan(t)), '%s: NaN pattern differs from the truth at %s' % (name, np.argwhere(np.isnan(g) != np.isnan(t))[:4].tolist())
    assert np.array_equal(g[np.isinf(t)], t[np.isinf(t)]), '%s: infinities differ' % name
    z = lambda a: np.where(fin, a, 0.0)
    if isinstance(atol, str):
        atol = rtol * float(np.abs(z(t)).max()) if t.size else 0.0
    k = cls or name.split(':')[0]
    if CAPS:   # the CPU test: the restatement itself must stay within the caps that keep the allowance from hiding a failure
        share, worst = ref_caps(name, r, t, rtol, atol)
        _CAPS[k] = (max(share, _CAPS.get(k, (0, 0))[0]), max(worst, _CAPS.get(k, (0, 0))[1]))
    rh, rr = assert_vs_truth(name, z(g), z(r), z(t), rtol, atol)
    if rh >= _WORST.get(k, (-1.0, 0.0))[0]:
        _WORST[k] = (rh, max(rr, _WORST.get(k, (0, 0.0))[1]))
    return rh, rr


def check_equal(name, got, want):
    got, want = (a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)) for a in (got, want))
    assert got.shape == want.shape and got.dtype == want.dtype, '%s: %s %s vs %s %s' % (name, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    if got.dtype.is_floating_point:   # bit for bit, NaN included
        got, want = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, '%s: %d elements differ, first at %s' % (name, bad.shape[0], bad[0].tolist())


def ref_caps(name, ref, truth, rtol, atol):
    """(share of the restatement's elements beyond half the bound, worst element / bound), asserted within the caps."""
    r, t = np.asarray(ref, dtype=F64), np.asarray(truth, dtype=F64)
    fin = np.isfinite(t)
    assert np.array_equal(np.isnan(r), np.isnan(t)), '%s: the restatement has another NaN pattern than the truth' % name
    if isinstance(atol, str):
        atol = rtol * float(np.abs(np.where(fin, t, 0)).max())
    with np.errstate(invalid='ignore'):
        ratio = np.where(fin, np.abs(np.where(fin, r - t, 0.0)), 0.0) / (rtol * np.where(fin, np.abs(t), 0.0) + atol + 1e-300)
    share, worst = float((ratio > 0.5).mean()) if ratio.size else 0.0, float(ratio.max()) if ratio.size else 0.0
    assert share <= MAX_SHARE and worst <= MAX_WORST, '%s: restatement %.2f %% beyond half the bound, worst x%.2f' % (name, 100 * share, worst)
    return share, worst


# ================================================================================================================= pe.hip
PE_FREQS = (0, 1, 4, 6, 10, 16)
PE_SCALES = (1.0, 0.5, 1.0 / 3.0)
PE_N = (1, 15, 16, 17, 257)
PE_SPECIAL = ((2, 0.0), (4, -0.0), (6, 1e-40), (8, np.inf), (10, -np.inf), (12, np.nan))   # (row, value) at component row % 3


def pe_width(nf):
    return 3 + 6 * nf


def _pe_case(kind, nf, n, stride, scale, mis=False, lim=1.0, **kw):
    c = dict(kind=kind, nf=nf, n=n, stride=stride, scale=scale, mis=mis, lim=lim, **kw)
    c['id'] = '%s f%d n%d s%d x%.2g%s%s%s' % (kind, nf, n, stride, scale, ' mis' if mis else '', ' |x|<=50' if lim > 1 else '',
                                            ' ' + kw['form'] if 'form' in kw else '')
    return c


def _pe_encode_cases():
    out, k = [], 0
    for nf in PE_FREQS:
        w = pe_width(nf)
        for stride in sorted({w, w + 1, 100} | ({64} if w <= 64 else set())):
            for mis in ((False, True) if stride == 64 else (False,)):
                out.append(_pe_case('enc', nf, PE_N[k % 5], stride, PE_SCALES[k % 3], mis, 50.0 if (nf == 16 and k % 2) else 1.0))
                k += 1
    # every n and every scale on each of the three paths (the rotation above does not promise it)
    for n, scale in itertools.product(PE_N, PE_SCALES):
        for stride, mis in ((39, False), (64, False), (64, True)):
            out.append(_pe_case('enc', 6, n, stride, scale, mis))
    out.append(_pe_case('enc', 16, 257, 100, 1.0 / 3.0, False, 50.0))
    seen, uniq = set(), []
    for c in out:
        if c['id'] not in seen:
            seen.add(c['id'])
            uniq.append(c)
    return uniq


PE_ENC_CASES = _pe_encode_cases()
PE_ENC_CAP_CASES = [_pe_case('enc', 6, 53774, 39, 0.5), _pe_case('enc', 6, 110000, 39, 1.0), _pe_case('enc', 10, 131073, 64, 1.0 / 3.0),
                    _pe_case('enc', 10, 131073, 64, 1.0, True)]
PE_JVP_CASES = [_pe_case('jvp', 6, 257, 64, 0.5), _pe_case('jvp', 6, 257, 64, 0.5, True), _pe_case('jvp', 6, 17, 39, 1.0 / 3.0)]
PE_JVP_CAP_CASES = [_pe_case('jvp', 6, 53774, 39, 0.5), _pe_case('jvp', 10, 131073, 64, 1.0), _pe_case('jvp', 10, 131073, 64, 0.5, True)]
PE_BWD_N = (1, 85, 86, 257)
PE_BWD_FORMS = ('one', 'two', 'zero')


def _pe_bwd_cases():
    out, k = [], 0
    for nf in PE_FREQS:
        for scale in PE_SCALES:
            out.append(_pe_case('bwd', nf, PE_BWD_N[k % 4], pe_width(nf) + (k % 3), scale, lim=50.0 if (nf == 16 and k % 2) else 1.0,
                                form=PE_BWD_FORMS[k % 3]))
            k += 1
    for n, form in itertools.product(PE_BWD_N, PE_BWD_FORMS):   # every n in every form
        out.append(_pe_case('bwd', 6, n, 64, 0.5, form=form))
    return out


PE_BWD_CASES = _pe_bwd_cases()
PE_BWD_CAP_CASES = [_pe_case('bwd', 6, 699051, 39, 0.5, form='one')]
APP_FREQS, APP_Q = (0, 4, 9), (1, 17, 257)
APP_CASES = [dict(kind='app', nf=nf, n=q, id='app f%d Q%d' % (nf, q)) for nf in APP_FREQS for q in APP_Q]
APP_CAP_CASES = [dict(kind='app', nf=4, n=131073, id='app f4 Q131073')]


def pe_path(c):
    """(kernel, passes of its grid-stride loop) -- psn_pe_encode / _jvp: the 64-column kernel iff out_stride == 64 and the output
    is 16-byte aligned (a view ``mis`` = one float into an aligned buffer is not); psn_pe_encode_bwd: one thread per (row,
    component); psn_app_input: one thread per four columns of 64."""
    if c['kind'] == 'bwd':
        kernel, items = 'bwd', c['n'] * 3
    elif c['kind'] == 'app':
        kernel, items = 'app', c['n'] * 16
    elif c['stride'] == 64 and not c['mis']:
        kernel, items = c['kind'] + '64', c['n'] * 16
    else:
        kernel, items = c['kind'] + ('_generic_from64' if c['stride'] == 64 else '_generic'), c['n'] * c['stride']
    blocks = min(-(-items // 256), GRID_CAP)
    return kernel, -(-items // (blocks * 256))


def pe_pass_rows(c):
    """[(pass, first row, end row)] of the rows that a pass of the capped grid writes at least partly."""
    kernel, passes = pe_path(c)
    per_row = {'bwd': 3, 'app': 16}.get(kernel, 16 if kernel in ('enc64', 'jvp64') else c.get('stride'))
    return [(p, p * PASS // per_row, min(c['n'], -(-((p + 1) * PASS) // per_row))) for p in range(passes)]


def pe_inputs(c):
    """x [n, 3] (cap cases: a 1024-row base tiled), tangent t for the JVP, gradient pieces for the backward."""
    n, nb = c['n'], min(c['n'], BASE_ROWS)
    g = rng(1, c['nf'], n, c.get('stride', 64))
    x = g.uniform(-c.get('lim', 1.0), c.get('lim', 1.0), (nb, 3)).astype(F32)
    special = []
    if c['kind'] in ('enc', 'jvp') and nb >= 15:
        for r, v in PE_SPECIAL:
            x[r, r % 3] = v
            special.append(r)
    inp = {'special': special, 'rows': np.arange(n) % nb}
    if c['kind'] == 'app':
        inp['p'], inp['v'], inp['nrm'] = x, (g.standard_normal((nb, 3)) * 3.0).astype(F32), g.standard_normal((nb, 3)).astype(F32)
        if nb >= 17:
            inp['v'][11] = 0.0
            inp['special'] = [11]
        return inp
    inp['x'] = x
    if c['kind'] == 'jvp':
        inp['t'] = g.standard_normal((nb, 3)).astype(F32)
    if c['kind'] == 'bwd':
        w, form = pe_width(c['nf']), c['form']
        inp['g1'] = g.standard_normal((nb, c['stride'] + 5)).astype(F32)   # the gradient is columns 2 .. 2 + stride of this
        inp['g2'] = g.standard_normal((nb, w + 9)).astype(F32) if form == 'two' else None   # columns 4 .. 4 + w
        if form == 'zero':
            inp['g1'][:] = 0.0
    return inp


def _bands(xs, nf, dtype, variant=None):
    """[(f, sin, cos)] of the fp32-rounded argument xs [n, 3] in float64 (truth) or float32 (torch.sin / torch.cos: restatement)."""
    out = []
    for f in range(nf):
        ff = f - 1 if (variant == 'last_band' and f == nf - 1) else f
        arg = np.ldexp(xs, ff).astype(F32)
        if variant == 'perm':
            arg = arg[:, [1, 2, 0]]
        with np.errstate(invalid='ignore'):
            if dtype is F64:
                s, co = np.sin(arg.astype(F64)), np.cos(arg.astype(F64))
            else:
                s, co = torch.sin(t32(arg)).numpy(), torch.cos(t32(arg)).numpy()
        if variant == 'swap' and f == nf // 2:
            s, co = co, s
        out.append((f, s, co))
    return out


def pe_encode_values(inp, c, dtype, variant=None):
    x, nf, stride = inp['x'], c['nf'], c['stride']
    xs = (x * F32(c['scale'])).astype(F32)
    out = np.zeros((x.shape[0], stride), dtype)
    if c['kind'] == 'enc':
        out[:, :3] = xs
        for f, s, co in _bands(xs, nf, dtype, variant):
            out[:, 3 + 6 * f:6 + 6 * f], out[:, 6 + 6 * f:9 + 6 * f] = s, co
        return out
    ts = (inp['t'] * F32(c['scale'])).astype(F32)
    out[:, :3] = ts
    for f, s, co in _bands(xs, nf, dtype, variant):
        with np.errstate(invalid='ignore', over='ignore'):
            out[:, 3 + 6 * f:6 + 6 * f] = np.ldexp((co * ts.astype(dtype)).astype(dtype), f)
            out[:, 6 + 6 * f:9 + 6 * f] = np.ldexp((-s * ts.astype(dtype)).astype(dtype), f)
    return out


def pe_bwd_pieces(inp, c):
    w = pe_width(c['nf'])
    g1 = inp['g1'][:, 2:2 + c['stride']]
    g2 = None if inp['g2'] is None else inp['g2'][:, 4:4 + w]
    return g1, g2


def pe_bwd_values(inp, c, dtype, variant=None):
    """d_x = scale * (g[c] + sum_f 2^f (cos(2^f xs) g_sin[f, c] - sin(2^f xs) g_cos[f, c])), g = g1 (+ g2)."""
    g1, g2 = pe_bwd_pieces(inp, c)
    g = g1.astype(dtype) if g2 is None else (g1.astype(dtype)[:, :g2.shape[1]] + g2.astype(dtype)).astype(dtype)
    xs = (inp['x'] * F32(c['scale'])).astype(F32)
    acc = g[:, :3].copy()
    for f, s, co in _bands(xs, c['nf'], dtype, 'perm' if variant == 'perm' else None):
        term = (co * g[:, 3 + 6 * f:6 + 6 * f]).astype(dtype) - (s * g[:, 6 + 6 * f:9 + 6 * f]).astype(dtype)
        acc = (acc + (term.astype(dtype) if variant == 'no_pow' else np.ldexp(term.astype(dtype), f))).astype(dtype)
    return acc if variant == 'no_scale' else (acc * dtype(F32(c['scale']))).astype(dtype)


def check_pe(c, inp, got):
    """got: [base rows, stride] (encode / JVP) or [base rows, 3] (backward) against truth and restatement; a pad column of the
    encode / JVP must be an exact zero."""
    fn = pe_bwd_values if c['kind'] == 'bwd' else pe_encode_values
    truth, ref = fn(inp, c, F64), fn(inp, c, F32)
    if c['kind'] == 'bwd':
        if c['form'] == 'zero':
            check_equal(c['id'] + ': zero gradient', torch.as_tensor(got), torch.zeros(truth.shape))
        return check('pe_%s: %s' % (c['kind'], c['id']), got, ref, truth, RTOL_GRAD, 'max')
    w = pe_width(c['nf'])
    g = np.asarray(got)
    assert not g[:, w:].any() and not np.signbit(g[:, w:]).any(), c['id'] + ': pad columns are not exact zeros'
    clean = np.ones(g.shape[0], bool)
    clean[inp['special']] = False
    assert np.isfinite(g[clean]).all(), c['id'] + ': a row next to a special one is not clean'
    if c['kind'] == 'jvp':   # 2^f |t| scale: the bound is relative to the band's magnitude
        return check('pe_jvp: ' + c['id'], got, ref, truth, RTOL_GRAD, 'max')
    return check('pe_enc: ' + c['id'], got, ref, truth, RTOL_VALUE, ATOL_UNIT)


# ---- appearance input table
def app_layout(nf):
    dv = pe_width(nf)
    return dict(p=(0, 3), vhat=(3, 6), bands=(6, 3 + dv), nrm=(3 + dv, 6 + dv), tail=(6 + dv, 64))


def app_vhat(inp, dtype):
    v = inp['v'].astype(dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        if dtype is F64:
            return v / np.sqrt((v * v).sum(1, keepdims=True))
        n2 = ((v[:, 0] * v[:, 0]).astype(F32) + (v[:, 1] * v[:, 1]).astype(F32)).astype(F32)
        n2 = (n2 + (v[:, 2] * v[:, 2]).astype(F32)).astype(F32)
        return (v / np.sqrt(n2).astype(F32)[:, None]).astype(F32)


def app_bands(vhat32, nf, dtype, variant=None):
    out = np.zeros((vhat32.shape[0], 6 * nf), dtype)
    for f, s, co in _bands(np.asarray(vhat32, dtype=F32), nf, dtype, variant):
        out[:, 6 * f:6 * f + 3], out[:, 6 * f + 3:6 * f + 6] = s, co
    return out


def check_app(c, inp, got):
    """got [base rows, 64].  p, n and the zero tail bit for bit; v^ against float64 v / |v|; the bands against float64 sin / cos
    of the table's own v^ columns.  A row with |v| = 0: NaN in its own view columns only (0 / 0, as torch.norm + division)."""
    lay, g = app_layout(c['nf']), np.asarray(got)
    check_equal(c['id'] + ': p', t32(g[:, 0:3]), t32(inp['p']))
    a, b = lay['nrm']
    check_equal(c['id'] + ': n', t32(g[:, a:b]), t32(inp['nrm']))
    assert not g[:, lay['tail'][0]:].any() and not np.signbit(g[:, lay['tail'][0]:]).any(), c['id'] + ': tail is not exact zeros'
    check('app_vhat: ' + c['id'], g[:, 3:6], app_vhat(inp, F32), app_vhat(inp, F64), RTOL_VALUE, ATOL_UNIT)
    if c['nf']:
        a, b = lay['bands']
        vh = g[:, 3:6].astype(F32)
        check('app_bands: ' + c['id'], g[:, a:b], app_bands(vh, c['nf'], F32), app_bands(vh, c['nf'], F64), RTOL_VALUE, ATOL_UNIT)


def app_restatement(c, inp, variant=None):
    lay = app_layout(c['nf'])
    out = np.zeros((inp['p'].shape[0], 64), F32)
    out[:, 0:3], out[:, 3:6] = inp['p'], app_vhat(inp, F32)
    out[:, lay['bands'][0]:lay['bands'][1]] = app_bands(out[:, 3:6], c['nf'], F32, variant)
    out[:, lay['nrm'][0]:lay['nrm'][1]] = inp['nrm']
    return out


# ======================================================================================================== weight_norm.hip
WN_WIDTHS = (1, 5, 63, 64, 65, 128, 289)
WN_ROWS = (1, 3, 4, 5, 257)
WN_MAX_ITEMS = 16
S2 = float(F32(1.0 / np.sqrt(2.0)))
EXACT_ROWS = ((3, 4), (1, 2, 2), (2, 3, 6))


def _it(rows, cols, scale=1.0, kind='rand', norm=1.0):
    return dict(rows=rows, cols=cols, scale=scale, kind=kind, norm=norm)


WN_CASES = [
    dict(id='widths x rows', items=[_it(r, w, (1.0, S2)[i % 2]) for i, (w, r) in enumerate(zip(WN_WIDTHS, (1, 3, 4, 5, 257, 3, 5)))]),
    dict(id='widths x rows, scales swapped', items=[_it(r, w, (S2, 1.0)[i % 2]) for i, (w, r) in enumerate(zip(WN_WIDTHS, (257, 5, 4, 3, 1, 4, 1)))]),
    dict(id='item boundaries inside a block', items=[_it(1, 5), _it(1, 65, S2), _it(1, 64), _it(1, 1, 0.5), _it(3, 63), _it(2, 128, S2), _it(7, 289)]),
    dict(id='16 items', items=[_it(1 + i % 5, WN_WIDTHS[i % 7], (1.0, S2)[i % 2]) for i in range(16)]),
    dict(id='17 items', items=[_it(1 + (i * 3) % 5, WN_WIDTHS[(i + 2) % 7], (S2, 1.0)[i % 2]) for i in range(17)]),
    dict(id='g zero and negative', items=[_it(5, 65, 1.0, 'gsign'), _it(4, 64, S2, 'gsign'), _it(3, 5, 1.0, 'gsign')]),
    dict(id='exact', items=[_it(r, w, s, 'exact') for (w, r), s in zip(zip(WN_WIDTHS, (3, 4, 5, 1, 257, 3, 4)), (1.0, 0.5, 1.0, 2.0, 0.25, 1.0, 0.5))]),
    dict(id='zero row', items=[_it(5, 65, 1.0, 'zero_row'), _it(4, 128, S2, 'zero_row'), _it(3, 5)]),
] + [dict(id='row norms %g' % nrm, items=[_it(r, w, (1.0, S2)[i % 2], 'rand', nrm) for i, (w, r) in enumerate(zip(WN_WIDTHS, (3, 4, 5, 1, 257, 5, 3)))])
     for nrm in (1e-6, 1.0, 1e6)]


def wn_path(case):
    """One wave per row, four rows per block, 64 lanes striding the columns; scale == 1 is a branch of the forward; lists longer
    than 16 items take a second launch.  -> set of path names."""
    paths = set()
    for c0 in range(0, len(case['items']), WN_MAX_ITEMS):
        chunk, row0, firsts = case['items'][c0:c0 + WN_MAX_ITEMS], 0, []
        for it in chunk:
            paths.add('scale==1' if it['scale'] == 1.0 else 'scale!=1')
            paths.add('cols%s64' % ('<' if it['cols'] < 64 else '==' if it['cols'] == 64 else '>'))
            paths.add('lane iterations %d' % -(-it['cols'] // 64))
            firsts.append(row0)
            row0 += it['rows']
        for a in firsts[1:]:
            if a % 4:
                paths.add('item boundary inside a block')
        per_block = {}
        for i, (a, it) in enumerate(zip(firsts, chunk)):
            for b in range(a // 4, (a + it['rows'] - 1) // 4 + 1):
                per_block.setdefault(b, set()).add(i)
        paths.add('items in one block: %d' % max(len(v) for v in per_block.values()))
        if row0 % 4:
            paths.add('last block partly idle')
        paths.add('%d items in a launch' % len(chunk))
    paths.add('launches %d' % -(-len(case['items']) // WN_MAX_ITEMS))
    return paths


def wn_inputs(case):
    """Per item (v [rows, cols], g [rows], dw [rows, cols]) float32."""
    out = []
    for i, it in enumerate(case['items']):
        g_ = rng(2, len(case['items']), i, it['rows'], it['cols'])
        rows, cols = it['rows'], it['cols']
        if it['kind'] == 'exact':
            v, dw = np.zeros((rows, cols), F32), g_.integers(-3, 4, (rows, cols)).astype(F32)
            for r in range(rows):
                vals = EXACT_ROWS[r % 3] if cols >= 3 else (3,)
                pos = [(r * 7 + k * (cols // len(vals))) % cols for k in range(len(vals))]   # spread over lanes and 64-column turns
                v[r, pos] = np.array(vals, F32) * (-1.0) ** (r + np.arange(len(vals)))
                if r % 4 == 3:
                    dw[r, pos] = 0.0   # dot = 0 exactly: the whole dv row is exact
            g = (2.0 ** g_.integers(-2, 3, rows)).astype(F32) * (-1.0) ** np.arange(rows)
        else:
            v = g_.standard_normal((rows, cols)).astype(F32)
            v = (v / np.sqrt((v.astype(F64) ** 2).sum(1, keepdims=True)) * it['norm']).astype(F32)
            dw = g_.standard_normal((rows, cols)).astype(F32)
            g = (g_.random(rows) + 0.5).astype(F32)
            if it['kind'] == 'gsign':
                g[0], g[-1] = 0.0, -g[-1]
                if rows > 2:
                    g[1] = -0.75
            if it['kind'] == 'zero_row':
                v[2] = 0.0
        out.append((v, g.astype(F32), dw))
    return out


def wn_truth(it, v, g, dw):
    v, g, dw, s = v.astype(F64), g.astype(F64)[:, None], dw.astype(F64), float(F32(it['scale']))
    with np.errstate(invalid='ignore', divide='ignore'):
        nrm = np.sqrt((v * v).sum(1, keepdims=True))
        dot = (dw * v).sum(1, keepdims=True) * s
        return dict(w=v * (g / nrm) * s, dv=dw * (g / nrm) * s - dot * g * v / nrm ** 3, dg=(dot / nrm)[:, 0], dv_term=dw * (g / nrm) * s)


def wn_torch32(it, v, g, dw, variant=None):
    """The torch formulation in float32: torch._weight_norm(v, g, 0) (nn.utils.weight_norm) [* scale] and its autograd."""
    tv, tg = t32(v).requires_grad_(), t32(g)[:, None].requires_grad_()
    w = torch._weight_norm(tv, tg, 0)   # what nn.utils.weight_norm evaluates
    if it['scale'] != 1.0:
        w = w * float(F32(it['scale']))
    w.backward(t32(dw))
    dv, dg = tv.grad.numpy(), tg.grad.numpy()[:, 0]
    if variant == 'dg_no_scale':
        dg = (dg / F32(it['scale'])).astype(F32)
    if variant == 'dv_no_projection':
        with np.errstate(invalid='ignore', divide='ignore'):
            dv = (dw * (g[:, None] / np.sqrt((v.astype(F64) ** 2).sum(1, keepdims=True))) * it['scale']).astype(F32)
    return dict(w=w.detach().numpy(), dv=dv, dg=dg)


def wn_kernel32(it, v, g, dw):
    """The kernel's own operation order in float32 with |v| from a float64 sum (exact for the exact cases): bit-equal where the
    module docstring says so."""
    s = F32(it['scale'])
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        nrm = np.sqrt((v.astype(F64) ** 2).sum(1)).astype(F32)
        sg = (g / nrm).astype(F32)
        w = (v * sg[:, None]).astype(F32)
        w = w if it['scale'] == 1.0 else (w * s).astype(F32)
        dot = ((dw.astype(F64) * v.astype(F64)).sum(1).astype(F32) * s).astype(F32)
        k = ((dot * g).astype(F32) / ((nrm * nrm).astype(F32) * nrm).astype(F32)).astype(F32)
        ss = (sg * s).astype(F32)
        dv = ((dw * ss[:, None]).astype(F32) - (k[:, None] * v).astype(F32)).astype(F32)
        return dict(w=w, dv=dv, dg=(dot / nrm).astype(F32), dot=dot)


def check_wn(case, inputs, got, only=('w', 'dv', 'dg')):
    """got: per item dict(w, dv, dg) of float32 arrays."""
    for i, (it, (v, g, dw), o) in enumerate(zip(case['items'], inputs, got)):
        truth, ref = wn_truth(it, v, g, dw), wn_torch32(it, v, g, dw)
        name = '%s [%d] %dx%d' % (case['id'], i, it['rows'], it['cols'])
        if it['kind'] == 'exact':
            k32 = wn_kernel32(it, v, g, dw)
            if 'w' in only:
                check_equal(name + ' w (exact)', t32(o['w']), t32(k32['w']))
            if 'dg' in only:
                check_equal(name + ' dg (exact)', t32(o['dg']), t32(k32['dg']))
            if 'dv' in only:
                ex = (v == 0) | (k32['dot'] == 0)[:, None]
                check_equal(name + ' dv (exact where v = 0 or dot = 0)', t32(np.where(ex, o['dv'], 0)), t32(np.where(ex, k32['dv'], 0)))
        t1 = truth['dv_term']
        atol_dv = RTOL_WN_BWD * float(np.abs(np.where(np.isfinite(t1), t1, 0)).max())
        for key, rtol, atol in (('w', RTOL_WN_FWD, 'max'), ('dv', RTOL_WN_BWD, atol_dv), ('dg', RTOL_WN_BWD, 'max')):
            if key in only:
                check('wn_%s: %s' % (key, name), o[key], ref[key], truth[key], rtol, atol)


# ============================================================================================================== small.hip
NORM_N = (1, 255, 256, 257)
NORM_EPS = (1e-12, 1e-3)
FLT_MAX = float(np.finfo(F32).max)


def norm_inputs(n, eps):
    """x, g [n, 3]: random rows at mixed magnitudes; from row 0 on (as many as fit) the special rows -- zero, norm below / at /
    just above eps (axis-aligned, so that fp32 and float64 agree on the branch), 1e-20, 1e18, 1e20 (the squares of 1e18 still
    fit fp32 -- 3e36 -- those of 1e20 overflow), a negative zero component, and random rows at 0.3 eps and 3 eps (more than one
    row on either side of the clamp)."""
    g_ = rng(3, n, int(-np.log10(eps)))
    e = F32(eps)
    x = (g_.standard_normal((n, 3)) * 10.0 ** g_.integers(-2, 3, (n, 1))).astype(F32)
    d = g_.standard_normal((8, 3))
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    sp = [np.zeros(3), [0.5 * e, 0, 0], [0, e, 0], [0, 0, np.nextafter(e, F32(1))], [1e-20, -1e-20, 1e-20], [1e18, 1e18, -1e18],
          [-0.0, 0.6, 0.8], d[0] * 0.3 * e, d[1] * 3 * e, d[2] * 0.3 * e, d[3] * 3 * e, [-0.7 * e, 0, 0], [1e20, -2e20, 1e20]]
    order = [6, 2, 0, 5, 1, 3, 4] + list(range(7, len(sp)))   # n = 1 takes the negative-zero row
    for r, k in enumerate(order[:n] if n < len(sp) else order):
        x[r] = np.asarray(sp[k], F64).astype(F32)
    return x, g_.standard_normal((n, 3)).astype(F32)


def _norm(x, dtype):
    x = x.astype(dtype)
    with np.errstate(over='ignore', under='ignore'):
        if dtype is F64:
            n2 = (x * x).sum(1)
            return np.where(n2 > FLT_MAX, np.inf, np.sqrt(n2))   # squares overflow fp32: the formulation's norm is +inf
        n2 = ((x[:, 0] * x[:, 0]).astype(F32) + (x[:, 1] * x[:, 1]).astype(F32)).astype(F32)
        return np.sqrt((n2 + (x[:, 2] * x[:, 2]).astype(F32)).astype(F32)).astype(F32)


def norm_fwd(x, eps, dtype):
    nrm = _norm(x, dtype)
    d = np.where(nrm < dtype(F32(eps)), dtype(F32(eps)), nrm).astype(dtype)
    return (x.astype(dtype) / d[:, None]).astype(dtype)


def norm_bwd(x, g, eps, dtype, variant=None):
    """autograd's chain of F.normalize (div -> clamp_min -> norm), in the kernel's order: dx = g / d + x / |x| * s,
    s = -sum_c (g_c x_c / d) / d, the second term only where |x| >= eps and |x| > 0."""
    nrm, e = _norm(x, dtype), dtype(F32(eps))
    d = np.where(nrm < e, e, nrm).astype(dtype)[:, None]
    x, g = x.astype(dtype), g.astype(dtype)
    with np.errstate(all='ignore'):
        out = (g / d).astype(dtype)
        q = (((g * x).astype(dtype) / d).astype(dtype) / d).astype(dtype)
        s = -((q[:, 0] + q[:, 1]).astype(dtype) + q[:, 2]).astype(dtype)
        live = (nrm > 0) if variant == 'ignore_clamp' else ((nrm >= e) & (nrm > 0))
        extra = ((x / np.where(live, nrm, 1)[:, None].astype(dtype)).astype(dtype) * s[:, None]).astype(dtype)
        return np.where(live[:, None], (out + extra).astype(dtype), out).astype(dtype)


def _row_scaled(*arrays):
    """Rows divided by max|truth row| (truth last): the per-row form of atol = rtol x max|truth|."""
    t = np.asarray(arrays[-1], dtype=F64)
    m = np.abs(np.where(np.isfinite(t), t, 0)).max(1, keepdims=True)
    m = np.where(m > 0, m, 1.0)
    return [np.asarray(a, dtype=F64) / m for a in arrays]


def check_norm(name, x, g, eps, y, dx):
    if y is not None:
        check('normalize_fwd: ' + name, y, norm_fwd(x, eps, F32), norm_fwd(x, eps, F64), RTOL_VALUE, ATOL_UNIT)
        big = (x.astype(F64) ** 2).sum(1) > FLT_MAX
        assert not np.asarray(y)[big].any(), name + ': a row whose squares overflow must normalise to exact zeros'
        clamp = _norm(x, F64) < float(F32(eps))
        check_equal(name + ': clamped rows are x / eps', t32(np.asarray(y)[clamp]), t32((x[clamp] / F32(eps)).astype(F32)))
    if dx is not None:
        a, r, t = _row_scaled(dx, norm_bwd(x, g, eps, F32), norm_bwd(x, g, eps, F64))
        check('normalize_bwd: ' + name, a, r, t, RTOL_GRAD, RTOL_GRAD)


# ---- light rows
LR_NIDX = (0, 1, 255, 256, 257, 513)
LR_TABLES = (1, 40, 256, 257, 600)
LR_MODES = ('dir', 'int', 'both')
LR_DUP_POS = (3, 255, 256, 512)
LR_CASES = [dict(n_idx=ni, n_rows=nr, mode=LR_MODES[(i + j) % 3], id='idx%d rows%d %s' % (ni, nr, LR_MODES[(i + j) % 3]))
            for i, ni in enumerate(LR_NIDX) for j, nr in enumerate(LR_TABLES)] + [
    dict(n_idx=513, n_rows=600, mode=m, id='idx513 rows600 %s' % m) for m in ('int', 'both')]


def lr_path(c):
    """(LDS chunks of 256 indices, blocks of 256 table rows, gradient pairs)."""
    return -(-c['n_idx'] // 256), -(-c['n_rows'] // 256), c['mode']


def lr_inputs(c):
    g_ = rng(4, c['n_idx'], c['n_rows'])
    tab = (g_.standard_normal((c['n_rows'], 3)) * 2.0).astype(F32)
    idx = g_.integers(0, c['n_rows'], c['n_idx']).astype(np.int64)
    dup = int(idx[3]) if c['n_idx'] > 3 else 0
    for p in LR_DUP_POS:   # the same row inside a chunk and across both chunk boundaries
        if p < c['n_idx']:
            idx[p] = dup
    return dict(tab=tab, itab=(g_.random((c['n_rows'], 1)) + 1.0).astype(F32), idx=idx, dup=dup,
                g_dir=g_.standard_normal((c['n_idx'], 3)).astype(F32), g_int=g_.standard_normal((c['n_idx'], 1)).astype(F32))


def lr_scatter_sum(idx, terms, n_rows, variant=None):
    """Dense table gradient: per table row the SEQUENTIAL float32 sum of its occurrences' terms in list order (from zero)."""
    out = np.zeros((n_rows, terms.shape[1]), F32)
    seen = set()
    for i, r in enumerate(idx.tolist()):
        if variant == 'first_duplicate_only' and r in seen:
            continue
        seen.add(r)
        out[r] = (out[r] + terms[i]).astype(F32)
    return out


def check_lr_bwd(c, inp, terms_dir, d_dir, d_int, variant=None):
    """d_dir against the sequential sum of ``terms_dir`` (the per-occurrence normalize backward [n_idx, 3] as float32: from the
    kernel under test on the GPU, from the restatement on the CPU), d_int against that of g_int: bit for bit, which includes the
    exact zeros of untouched rows and of a whole table at n_idx = 0."""
    touched = np.zeros(c['n_rows'], bool)
    touched[inp['idx']] = True
    if d_dir is not None:
        check_equal(c['id'] + ': d_dir', t32(d_dir), t32(lr_scatter_sum(inp['idx'], terms_dir, c['n_rows'])))
        assert not np.asarray(d_dir)[~touched].any()
    if d_int is not None:
        check_equal(c['id'] + ': d_int', t32(d_int), t32(lr_scatter_sum(inp['idx'], inp['g_int'], c['n_rows'])))
        assert not np.asarray(d_int)[~touched].any()


# ---- camera rays
CAM_CASES = [dict(n=n, idx=ix, scale=s, id='n%d %s scale%+d' % (n, 'idx' if ix else 'all', s))
             for k, (n, ix) in enumerate(itertools.product((1, 256, 257), (False, True))) for s in ((1.0, -1.0) if n == 257 else ((1.0, -1.0)[k % 2],))]


def cam_inputs(c):
    g_ = rng(5, c['n'], c['idx'])
    P = c['n'] + 44 if c['idx'] else c['n']
    uv = np.stack([g_.integers(0, 612, P), g_.integers(0, 512, P)], -1).astype(F32)[None]
    K = np.eye(4, dtype=F32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 3759.0, 3741.5, 306.25, 255.5
    a, b = np.radians(40.0), np.radians(-15.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    pose = np.eye(4, dtype=F32)
    pose[:3, :3], pose[:3, 3] = (Rz @ Rx).astype(F32), [3.0, -2.0, 31.5]
    idx = np.sort(g_.permutation(P)[:c['n']]).astype(np.int64) if c['idx'] else None
    return dict(uv=uv, K=K[None], pose=pose[None], idx=idx)


def cam_values(inp, c, dtype, variant=None):
    uv = inp['uv'][0] if inp['idx'] is None else inp['uv'][0][inp['idx']]
    K, R = inp['K'][0].astype(dtype), inp['pose'][0].astype(dtype)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if variant == 'perm':
        cx, cy = cy, cx
    r = lambda a: a.astype(dtype)
    x = r(r(uv[:, 0].astype(dtype) - cx) / fx)
    y = r(r(uv[:, 1].astype(dtype) - cy) / fy)
    d = np.stack([r(r(r(x * R[k, 0]) + r(y * R[k, 1])) + R[k, 2]) for k in range(3)], -1)
    if dtype is F64:
        return d / np.sqrt((d * d).sum(1, keepdims=True)) * c['scale']
    return (norm_fwd(d, 1e-12, F32) * F32(c['scale'])).astype(F32)


# ---- mask count
MC_N = (0, 1, 7, 8, 9, 1023, 8191, 2 ** 24 - 1)
MC_BYTES = (1, 2, 0x7f, 0x80, 0xff)
MC_ALIGN = ((0, 0), (0, 1), (1, 0), (0, None), (1, None), (8, 16))   # byte offsets of a and b from an 8-byte boundary; None: no b
MC_CASES = [dict(n=n, off=al, id='n%d a+%s b+%s' % (n, al[0], al[1])) for n in MC_N for al in MC_ALIGN
            if n < 2 ** 20 or al in ((0, 0), (0, 1))]   # (the 16 MB masks: one case per path)


def mc_path(c):
    """'words' (eight bytes per load + byte tail) iff both pointers are 8-byte aligned (an absent b counts as aligned)."""
    a, b = c['off']
    words = a % 8 == 0 and (b is None or b % 8 == 0)
    return ('words' if words else 'bytes'), ('tail' if (c['n'] % 8 if words else c['n']) else 'no tail'), ('b' if b is not None else 'no b')


def mc_inputs(c):
    g_ = rng(6, c['n'], c['off'][0], 99 if c['off'][1] is None else c['off'][1])
    val = np.array((0,) + MC_BYTES, np.uint8)
    a = val[g_.integers(0, 6, c['n'])] * (g_.random(c['n']) < 0.7)
    b = None if c['off'][1] is None else (val[g_.integers(0, 6, c['n'])] * (g_.random(c['n']) < 0.8)).astype(np.uint8)
    return a.astype(np.uint8), b


def mc_truth(a, b):
    return float(np.count_nonzero((a != 0) & (True if b is None else (b != 0))))


# ---- surface index / inverse index
SI_N = (0, 1, 1023, 1024, 1025, 5000)
SI_MASKS = ('empty', 'full', 'last', 'random')
SI_CASES = [dict(n=n, mask=m, cap=cp, id='n%d %s cap %s' % (n, m, cp)) for n in SI_N for m in SI_MASKS for cp in ('below', 'at', 'above')
            if not (n == 0 and m != 'empty')]


def si_inputs(c):
    n = c['n']
    m = {'empty': np.zeros(n, bool), 'full': np.ones(n, bool), 'last': np.arange(n) == n - 1,
         'random': rng(8, n).random(n) < 0.4}[c['mask']]
    byt = np.where(m, np.array(MC_BYTES, np.uint8)[np.arange(n) % 5], 0).astype(np.uint8)   # any non-zero byte is set
    live = int(m.sum())
    cap = {'below': max(1, live - 1 - live // 3), 'at': max(1, live), 'above': live + 1 + 1024 * (n >= 1024)}[c['cap']]
    return byt, cap


def si_path(c):
    byt, cap = si_inputs(c)
    live, q = int(np.count_nonzero(byt)), -(-c['n'] // 1024)
    return ('bytes per thread %d' % q, 'idle threads' if (-(-c['n'] // q) if q else 0) < 1024 else 'all threads',
            'truncated' if cap < live else 'padded' if cap > live else 'exact fit', 'empty' if live == 0 else 'live')


def si_truth(byt, cap):
    nz = np.flatnonzero(byt).astype(np.int64)
    idx = np.full(cap, nz[-1] if nz.size else 0, np.int64)
    idx[:min(cap, nz.size)] = nz[:cap]
    return idx, float(nz.size)


II_NPIX = (1, 256, 257)
II_COUNTS = ('none', 'zero', 'below', 'equal', 'above')
II_CASES = [dict(n_pix=n, count=cn, pad=pd, id='pix%d count %s%s' % (n, cn, ' padded' if pd else '')) for n in II_NPIX for cn in II_COUNTS for pd in (False, True)]


def ii_inputs(c):
    """(idx: ascending pixel list, padded by repeats of its last entry when asked, count or None)."""
    n = c['n_pix']
    m = rng(9, n).random(n) < 0.5
    m[n - 1] = n == 1 or m[n - 1]
    nz = np.flatnonzero(m).astype(np.int64)
    live = nz.size
    idx = np.concatenate([nz, np.full(5 if c['pad'] else 0, nz[-1] if live else 0, np.int64)])
    count = {'none': None, 'zero': 0.0, 'below': float(max(live - 2, 0)), 'equal': float(live), 'above': float(idx.size + 3)}[c['count']]
    return idx, count


def ii_truth(idx, count, n_pix, variant=None):
    ns = idx.size if count is None else min(int(count), idx.size)
    inv = np.full(n_pix, -1, np.int32)
    order = range(ns) if variant == 'last_repeat' else range(ns - 1, -1, -1)   # the FIRST of equal entries wins
    for k in order:
        inv[idx[k]] = k
    return inv


# ---- copy2d group
C2_MAX = 24
C2_COUNTS = (1, 255, 256, 257)


def _c2(rows, cols, pad_src, pad_dst, one_d=False):
    return dict(rows=rows, cols=cols, ld_src=cols + pad_src, ld_dst=cols + pad_dst, one_d=one_d)


C2_CASES = [
    dict(id='1-D items', items=[_c2(1, e, 0, 0, True) for e in C2_COUNTS]),
    dict(id='2-D ld > cols either side', items=[_c2(r, cc, ps, pd) for (r, cc), (ps, pd) in zip(((1, 1), (5, 51), (16, 16), (257, 1), (3, 85), (1, 257), (17, 15)),
                                                                                            ((3, 0), (0, 2), (1, 1), (0, 4), (7, 0), (2, 2), (0, 0)))]),
    dict(id='16 items', items=[_c2(1 + i % 4, C2_COUNTS[i % 4], i % 3, (i + 1) % 3) for i in range(16)]),
    dict(id='17 items', items=[_c2(1 + i % 3, C2_COUNTS[(i + 1) % 4], (i + 2) % 3, i % 2) for i in range(17)]),
    dict(id='24 items', items=[_c2(1 + i % 2, 1 + 37 * i, i % 2, 1) for i in range(24)]),
    dict(id='25 items', items=[_c2(2, 128 + i, 1, i % 2) for i in range(25)]),
]


def c2_path(case):
    paths = set()
    for c0 in range(0, len(case['items']), C2_MAX):
        chunk = case['items'][c0:c0 + C2_MAX]
        paths.add('%d items in a launch' % len(chunk))
        for it in chunk:
            e = it['rows'] * it['cols']
            paths.add('1-D' if it['one_d'] else '2-D')
            paths.add('elements %s 256' % ('<' if e < 256 else '==' if e == 256 else '>'))
            if it['ld_src'] > it['cols']:
                paths.add('ld_src > cols')
            if it['ld_dst'] > it['cols']:
                paths.add('ld_dst > cols')
    paths.add('launches %d' % -(-len(case['items']) // C2_MAX))
    return paths


# ============================================================================================================== views.hip
VB_H, VB_W, VB_LV, VB_R = 23, 37, 8, 5
VB_HW = VB_H * VB_W
VB_TYPES = ('float32', 'uint8', 'uint16')
VB_N = (1, 255, 256, 257, 513)
VB_PIX = ('list', 'range0', 'range7')
VB_L = (1, 4, 96)
VB_OUTPUTS = ('rgb', 'object_mask', 'surface_mask', 'uv', 'points', 'normal', 'visibility', 'vis_train_gt', 'sampling_idx', 'light_direction')


def _vb(dtype, n, pix, L, vis, V, view=0, drop=None):
    c = dict(dtype=dtype, n=n, pix=pix, L=L, vis=vis, V=V, view=view, drop=drop)
    c['id'] = '%s n%d %s L%d %s V%d view%d%s' % (dtype, n, pix, L, 'vis' if vis else 'novis', V, view, ' -' + drop if drop else '')
    return c


def _vb_cases():
    out, k = [], 0
    for dtype in VB_TYPES:
        for n in VB_N:
            for vis, V in ((True, 0), (True, 3), (False, 0), (False, 3)):
                if (k + vis + V) % 2 and not (n == 257):   # half of the (vis, V) grid per (type, n); all four at n = 257
                    k += 1
                    continue
                out.append(_vb(dtype, n, VB_PIX[k % 3], VB_L[(k // 2) % 3] if n > 1 else 96, vis, V, k % 2))
                k += 1
    for dtype in VB_TYPES:
        for pix in VB_PIX:
            out.append(_vb(dtype, 1, pix, 96, True, 3, 1))       # 3 L = 288 > 256 threads: the light-direction loop iterates twice
            out.append(_vb(dtype, 255, pix, 96, False, 3, 0))
            out.append(_vb(dtype, 513, pix, 4, True, 3, 1))
        out.append(_vb(dtype, 257, 'list', 0, False, 0, 0))      # attributes only
        out.append(_vb(dtype, 257, 'range7', 0, False, 3, 1))
    for drop in VB_OUTPUTS[1:]:                                  # (rgb cannot be left out: the entry point requires it when n_lights > 0)
        out.append(_vb('uint8', 257, 'list', 4, drop != 'visibility', 0 if drop == 'vis_train_gt' else 3, 0, drop))
    seen, uniq = set(), []
    for c in out:
        if c['id'] not in seen:
            seen.add(c['id'])
            uniq.append(c)
    return uniq


VB_CASES = _vb_cases()


def vb_path(c):
    """(image type, pixel source, job kinds along blockIdx.y, iterations of the light-direction loop, whether the vis_train_gt
    jobs are numbered behind visibility jobs (Lv = L) or directly behind the attribute job (Lv = 0))."""
    jobs = ['attr'] + (['rgb'] if c['L'] else []) + (['vis'] if c['vis'] and c['L'] else []) + (['vtg'] if c['V'] else [])
    threads = -(-c['n'] // 256) * 256
    ld = 0 if (c['drop'] == 'light_direction' or c['L'] == 0) else -(-3 * c['L'] // threads)
    shift = None if not c['V'] else ('Lv=L' if (c['vis'] and c['L']) else 'Lv=0')
    return c['dtype'], ('list' if c['pix'] == 'list' else 'pix0=0' if c['pix'] == 'range0' else 'pix0>0'), tuple(sorted(jobs)), ld, shift


def vb_tables(view, dtype):
    g_ = rng(10, view)
    f = lambda *s: g_.standard_normal(s).astype(F32)
    t = dict(width=VB_W, object_mask=g_.random(VB_HW) < 0.7, surface_mask=g_.random(VB_HW) < 0.5, points=f(VB_HW, 3), normal=f(VB_HW, 3),
             visibility=g_.random((VB_LV, VB_HW)).astype(F32), vis_plus=g_.random((VB_R, VB_HW)).astype(F32), light_direction=f(VB_LV, 3))
    if dtype == 'float32':
        t['images'] = g_.random((VB_LV, VB_HW, 3)).astype(F32)
    else:
        size = 256 if dtype == 'uint8' else 65536
        t['images'] = g_.integers(0, size, (VB_LV, VB_HW, 3)).astype(np.uint8 if dtype == 'uint8' else np.uint16)
        t['lut'] = rng(11, size).random(size).astype(F32)   # NOT k / 255: a mix-up of tables or types shows
    return t


def vb_indices(c):
    g_ = rng(12, c['n'], c['L'], c['view'])
    lidx = {0: np.zeros(0, np.int64), 1: np.array([6]), 4: np.array([5, 2, 5, 0]), 96: (np.arange(96) * 5 + 3) % VB_LV}[c['L']].astype(np.int64)
    pix0 = {'list': 0, 'range0': 0, 'range7': 7}[c['pix']]
    pix = g_.integers(0, VB_HW, c['n']).astype(np.int64) if c['pix'] == 'list' else None   # unsorted, with repeats
    vidx = np.array([4, 0, 4], np.int64)[:c['V']]
    return lidx, pix, pix0, vidx


def vb_truth(c, t, variant=None):
    """Every output by numpy indexing: dict name -> array (the outputs the case asks for)."""
    lidx, pix, pix0, vidx = vb_indices(c)
    px = pix if pix is not None else pix0 + np.arange(c['n'], dtype=np.int64)
    img = t['images'] if c['dtype'] == 'float32' else t['lut'][t['images'].astype(np.int64)]
    om = t['object_mask'][px]
    out = {'object_mask': om, 'surface_mask': t['surface_mask'][px], 'points': t['points'][px], 'normal': t['normal'][px], 'sampling_idx': px,
           'uv': np.stack([px % VB_W, px // VB_W], -1).astype(F32)}
    if c['L']:
        rgb = img[lidx][:, px]
        out['rgb'] = rgb if variant == 'no_mask' else (rgb * om[None, :, None].astype(F32)).astype(F32)
        out['light_direction'] = t['light_direction'][lidx]
        if c['vis']:
            out['visibility'] = t['visibility'][np.arange(c['L']) % VB_LV if variant == 'vis_row_l' else lidx][:, px]
    if c['V']:
        out['vis_train_gt'] = t['vis_plus'][vidx][:, px]
    out.pop(c['drop'], None)
    return out


def check_vb(c, got, want):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in want:
        check_equal('%s: %s' % (c['id'], k), torch.as_tensor(np.asarray(got[k])), torch.as_tensor(np.asarray(want[k])))
