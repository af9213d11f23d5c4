"""The GEMM family (csrc/gemm.hip) against float64 and exact integers, path by path, on the cases of tests/gemm_cases.py (whose
coverage of the dispatchers tests/test_gemm_cpu.py asserts without a GPU, through psn_gemm_plan / psn_gemm_tn_plan /
psn_colsum_plan): gemm_kernel<TA,TB,2|4> with every epilogue and every vector / scalar fallback of its operands, split-K and its
two reductions, the grouped weight-gradient launch with its 128 x 128-tile, 256 x 256-tile (register-staged, LDS-DMA and
split-bf16) and 256 x 64-tile kernels in every loop regime, table operands on both sides of the 2^24 threshold of the
reciprocal division, groups of several launches, and psn_colsum on both sides of its 256-column cap.

Two operand classes per case.  'int': small integers, every partial sum exact in fp32 -- the kernel must EQUAL the float64
result (torch.equal) on C, on every side output and on the column sums: every k row used exactly once, at no tolerance.
'real': randn operands under helpers.assert_vs_truth(rtol 1e-5, 'max') with the float32 CPU definition as the reference
arithmetic (the nonlinear outputs with the rtol of test_gemm_epilogues_and_strides: gemm_cases.RTOL_OUT); test_gemm_cpu.py shows
that this reference never passes half the bound, so the kernel is allowed no element beyond it.  Every operand is a view into a
buffer of NaNs of a fixed bit pattern: what a kernel reads from outside its operands poisons the result, what it must not write
keeps its bits.  Every grouped call runs twice and is bit-identical.

Measured worst r_hip per instantiation (units of the bound) on an MI355X; the 'int' class has no figure, it is bit-equal:
    instantiation                           r_hip   r_ref   worst tensor
    gemm_kernel<NN,2>                       0.093   0.093   C-nt2-NN-257x217x33-BIAS_SIGMOID-C_ld C
    gemm_kernel<NN,4>                       0.018   0.018   B-rows-NN-262017x132x33-NONE C
    gemm_kernel<NT,2>                       0.118   0.113   C-nt2-NT-257x217x33-BIAS_SIGMOID-C_ld C
    gemm_kernel<NT,4>                       0.081   0.086   C-nt4-NT-262017x256x16-BIAS_SIGMOID C
    gemm_kernel<TN,2>                       0.027   0.021   A-mis-TN-128x3x126-NONE-A_base C
    gemm_kernel<TN,2> colsum                0.009   0.010   D-seam-TN-256x217x48-NONE-s2-cs colsum
    gemm_kernel<TN,4>                       0.098   0.093   C-nt4-TN-262017x217x17-BIAS_SIGMOID-C_ld C
    gemm_kernel<TN,4> colsum                0.064   0.014   B-split-TN-256x255x16384-ACCUM-s1024-cs colsum
    gemm_kernel<TT,2>                       0.032   0.032   A-pair-TT-129x128x126-NONE C
    gemm_kernel<TT,4>                       0.018   0.018   B-rows-TT-262017x256x33-NONE C
    gemm_tn256_grouped_kernel DMA           0.048   0.029   E-217x256-K513 item 0
    gemm_tn256_grouped_kernel DMA colsum    0.017   0.010   E-217x256-K513 item 1
    gemm_tn256_grouped_kernel staged        0.043   0.043   E-256x200-K161 item 0
    gemm_tn256_grouped_kernel staged colsum 0.019   0.011   E-256x200-K4099 item 1
    gemm_tn_grouped_kernel                  0.046   0.038   G-fallback-K513 item 1
    gemm_tn_grouped_kernel colsum           0.012   0.011   G-tile-split-K4099 item 2
    gemm_tn_tall_grouped_kernel             0.043   0.035   F-130x33-K513 item 0
    gemm_tn_tall_grouped_kernel colsum      0.014   0.010   F-256x64-K193 item 2
    colsum_partial_kernel<0 | 1 | 3 | 4>    0.029 | 0.032 | 0.033 | 0.026
    colsum_partial_vec_kernel<0 | 1 | 3 | 4>  0.012 | 0.009 | 0.012 | 0.026
1836 tests, 94 s of wall time for the module, most of it building operands and float64 results on the host.  The ceiling
cases: gemm_kernel<.,.,4> at M = 262,017 (family B and the NT = 4 half of family C) 1.5 - 3.4 s per test, the table cases at K
near 2^24 2.0 s each (with A = [K, 1]; 11 s with A = [K, 4], which is why M is 1 there), everything else well below a second.

Findings of this suite.  No kernel and no launcher of gemm.hip was found wrong: the clamped loads of the 256 x 256- and
256 x 64-tile kernels meet NaN guards on every side and no NaN reaches a stored element, fastdiv24 is exact for every divisor
of the table (1, 2, 3, 7, 777, 4096, with and without a wrapping modulo) up to k = 2^24 - 1, and the integer-division branch
above it agrees.  Two defects of the binding, both at M = 0 (fixed in psnerf_amd/hip.py, cases H-0x* kept): hip.colsum raised
"null pointer" for an empty X -- an empty tensor has no address, and psn_colsum, which defines the result as zeros or as the
unchanged output, never got to run -- and row_weight.reshape(0, -1) raised before that.
"""
import collections
import time

import pytest
import torch

from tests import gemm_cases as gc

pytestmark = pytest.mark.gpu
_WORST = {}      # instantiation -> (worst r_hip, r_ref there, case and tensor)
_SLOW = []       # (seconds, test) of the slowest tests
_T0 = [None]
LAYOUT_NAME = {(False, True): 'NT', (False, False): 'NN', (True, False): 'TN', (True, True): 'TT'}


@pytest.fixture(scope='module', autouse=True)
def _report():
    _T0[0] = time.time()
    yield
    if _WORST:
        print('\n==== GEMM family vs float64: worst r_hip per instantiation (r_ref in the same tensor), in units of the bound ====')
        for name, (rh, rr, where) in sorted(_WORST.items()):
            print('%-36s r_hip %6.3f  r_ref %6.3f  (%s)' % (name, rh, rr, where))
    print('module wall time %.1f s; slowest tests:' % (time.time() - _T0[0]))
    for sec, name in sorted(_SLOW, reverse=True)[:8]:
        print('  %6.2f s  %s' % (sec, name))


@pytest.fixture(autouse=True)
def _timed(request):
    t = time.time()
    yield
    _SLOW.append((time.time() - t, request.node.name))


@pytest.fixture(scope='module')
def hip(cuda):
    from psnerf_amd import hip
    return hip


def record(path, where, rh, rr):
    if rh > _WORST.get(path, (-1.0,))[0]:
        _WORST[path] = (rh, rr, where)


def same_placement(dev, cpu):
    """The device view sits like the CPU view the plan query was asked about."""
    return dev.data_ptr() % 16 == cpu.data_ptr() % 16 and dev.stride() == cpu.stride() and dev.shape == cpu.shape


# --------------------------------------------------------------------------- psn_gemm: families A - D
def call_gemm(hip, c, buf, **override):
    g = lambda name: buf[name][1] if name in buf else None
    kw = dict(trans_a=c['ta'], trans_b=c['tb'], bias=g('bias'), epi=gc.EPI[c['epi']], aux_in=g('aux1'), out=g('C'), aux_out=g('aux_out'),
              split_k=c['split_k'], aux_in2=g('aux2'), colsum_a=g('colsum'))
    kw.update(override)
    return hip.gemm(g('A'), g('B'), **kw)


GEMM_RUNS = [(c, cls) for c in gc.GEMM_CASES for cls in c['classes']]


@pytest.mark.parametrize('c,cls', GEMM_RUNS, ids=['%s-%s' % (c['id'], cls) for c, cls in GEMM_RUNS])
def test_gemm(hip, cuda, c, cls):
    op = gc.build_gemm(c, cls)
    cpu_buf = gc.gemm_buffers(op)
    buf = {k: (w.to(cuda), None) for k, (w, _) in cpu_buf.items()}
    M, N, m = c['M'], c['N'], c['modes']
    for k, (w, _) in buf.items():       # re-slice the views on the device
        v = cpu_buf[k][1]
        mode = m.get(k)
        buf[k] = (w, gc.vec_of(w, v.numel()) if v.dim() == 1 else gc.view_of(w, v.shape[0], v.shape[1], mode))
        assert same_placement(buf[k][1], v), k
    pl = gc.gemm_plan_of(c)
    path = 'gemm_kernel<%s,%d>' % (LAYOUT_NAME[(c['ta'], c['tb'])], pl.bn // 64)
    del cpu_buf
    out = call_gemm(hip, c, buf)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf['C'][1].data_ptr()
    # what the call must not write keeps its bits
    assert gc.guards_intact(buf['C'][0], M, N, m['C']), 'C guards'
    if 'aux_out' in buf:
        assert gc.guards_intact(buf['aux_out'][0], M, N, m['aux_out']), 'aux_out guards'
    if 'colsum' in buf:
        assert gc.vec_guards_intact(buf['colsum'][0], M), 'colsum guards'
    got = {'C': buf['C'][1].cpu(), 'aux_out': buf['aux_out'][1].cpu() if 'aux_out' in buf else None,
           'colsum': buf['colsum'][1].cpu() if 'colsum' in buf else None}
    del buf
    outs = gc.gemm_outputs(c)
    blocks = gc.row_blocks(M)
    cut = lambda name, rows: got[name] if (name == 'colsum' or len(blocks) == 1) else got[name][rows]
    assert len(blocks) == 1 or not c['colsum']
    if cls == 'int':
        for rows in blocks:
            truth = gc.gemm_def(op, torch.float64, rows)
            for name, i, _ in outs:
                gc.check_int('%s %s' % (c['id'], name), cut(name, rows), truth[i])
        return
    if len(blocks) == 1:
        truth, ref = gc.gemm_def(op, torch.float64), gc.gemm_def(op, torch.float32)
        for name, i, rtol in outs:
            rh, rr = gc.check_real('%s %s' % (c['id'], name), got[name], ref[i], truth[i], rtol)
            record(path if name != 'colsum' else path + ' colsum', '%s %s' % (c['id'], name), rh, rr)
        return
    tmax = collections.defaultdict(float)       # block by block: the maximum of the truth first, the ratios after it
    for rows in blocks:
        truth = gc.gemm_def(op, torch.float64, rows)
        for name, i, _ in outs:
            tmax[name] = max(tmax[name], float(truth[i].abs().max()))
    for rows in blocks:
        truth, ref = gc.gemm_def(op, torch.float64, rows), gc.gemm_def(op, torch.float32, rows)
        for name, i, rtol in outs:
            rh, rr = gc.check_real('%s %s rows %d..' % (c['id'], name, rows.start), got[name][rows], ref[i], truth[i], rtol,
                                   atol=rtol * tmax[name])
            record(path, '%s %s' % (c['id'], name), rh, rr)


@pytest.mark.parametrize('name,epi,what', gc.ARG_CHECKS, ids=[a[0] for a in gc.ARG_CHECKS])
def test_gemm_argument_checks(hip, cuda, name, epi, what):
    """A missing aux_in / aux_in2 / aux_out / bias, split_k > 1 with an epilogue other than NONE / ACCUM, colsum_a without
    trans_a: RuntimeError, and nothing is written."""
    c = gc.gemm_case('X', name, False, True, 130, 132, 33, epi=epi, colsum=what == 'colsum', classes=('real',))
    c['aux_out'] = True
    op = gc.build_gemm(c, 'real')
    buf = {}
    for k, (w, v) in gc.gemm_buffers(op).items():
        w = w.to(cuda)
        buf[k] = (w, gc.vec_of(w, v.numel()) if v.dim() == 1 else gc.view_of(w, v.shape[0], v.shape[1], 'ok'))
    override = {'split': dict(split_k=2), 'colsum': {}, 'aux1': dict(aux_in=None), 'aux2': dict(aux_in2=None),
                'aux_out': dict(aux_out=None), 'bias': dict(bias=None)}[what]
    with pytest.raises(RuntimeError):
        call_gemm(hip, c, buf, **override)
    torch.cuda.synchronize()
    for k in ('C', 'aux_out', 'colsum'):
        if k in buf:
            assert gc.untouched(buf[k][0]), k


# --------------------------------------------------------------------------- psn_gemm_tn_grouped: families E - G
KIND_NAME = {0: 'gemm_tn_grouped_kernel', 1: 'gemm_tn256_grouped_kernel', 2: 'gemm_tn_tall_grouped_kernel'}
X3_MODES = {6: 'bf16x6', 3: 'bf16x3', 1: 'bf16'}
TN_RUNS = [(c, cls, 0) for c in gc.TN_CASES for cls in c['classes']] + \
          [(c, 'int', p) for c in gc.TN_CASES if c['x3'] for p in (6, 3, 1)]


def launch_tn(hip, cuda, c, cpu_items, products):
    dev = gc.tn_to(c, cpu_items, lambda t: t.to(cuda))
    if products:
        with hip.wgrad_precision(X3_MODES[products]):
            res = hip.gemm_tn_grouped(dev, c['split_k'], x3=True)
    else:
        res = hip.gemm_tn_grouped(dev, c['split_k'], x3=False)
    torch.cuda.synchronize()
    return dev, res


@pytest.mark.parametrize('c,cls,products', TN_RUNS, ids=['%s-%s%s' % (c['id'], cls, '-x3p%d' % p if p else '') for c, cls, p in TN_RUNS])
def test_gemm_tn_grouped(hip, cuda, c, cls, products):
    """products = 0: the fp32 kernels; 6 / 3 / 1: the 256 x 256-tile items through the split-bf16 kernel with that many partial
    products ('int' only: an 8-bit integer is its own hi plane, so the result is exact with any of them)."""
    K = c['K']
    cpu_items = gc.build_tn(c, cls)
    kinds = []
    for chunk in gc.tn_chunks(cpu_items):
        pl = hip.gemm_tn_plan(chunk, c['split_k'])
        kinds += [(pl.kind[i], pl.dma[i]) for i in range(len(chunk))]
    dev, res = launch_tn(hip, cuda, c, cpu_items, products)
    for n, (it, d, (C, cs)) in enumerate(zip(cpu_items, dev, res)):
        s = it['spec']
        for name in gc.TN_OPERANDS:
            if name in it['whole']:
                assert same_placement(d[name], it[name]), '%s item %d %s' % (c['id'], n, name)
        assert C.data_ptr() == d['out'].data_ptr() and (cs is not None) == bool(s['colsum'])
        assert gc.guards_intact(d['whole']['out'], s['M'], s['N'], s['C']), 'item %d: guards of the result' % n
        truth = gc.tn_item_def(it, K, torch.float64)
        where = '%s item %d' % (c['id'], n)
        kind, dma = kinds[n]
        path = KIND_NAME[kind] + ((' DMA' if dma else ' staged') if kind == 1 else '')
        if cls == 'int':
            gc.check_int(where, C, truth[0])
            if cs is not None:
                gc.check_int(where + ' colsum', cs, truth[1])
        else:
            ref = gc.tn_item_def(it, K, torch.float32)
            record(path, where, *gc.check_real(where, C, ref[0], truth[0], gc.RTOL))
            if cs is not None:
                record(path + ' colsum', where, *gc.check_real(where + ' colsum', cs, ref[1], truth[1], gc.RTOL))
    # the same call again (fresh result buffers: some items accumulate): bit-identical, fixed summation order
    dev2, res2 = launch_tn(hip, cuda, c, cpu_items, products)
    for n, ((C, cs), (C2, cs2)) in enumerate(zip(res, res2)):
        assert torch.equal(C.view(torch.int32), C2.view(torch.int32)), 'item %d is not deterministic' % n
        assert cs is None or torch.equal(cs.view(torch.int32), cs2.view(torch.int32)), 'colsum of item %d is not deterministic' % n


# --------------------------------------------------------------------------- psn_colsum: family H
COLSUM_RUNS = [(c, cls) for c in gc.COLSUM_CASES for cls in c['classes']]


@pytest.mark.parametrize('c,cls', COLSUM_RUNS, ids=['%s-%s' % (c['id'], cls) for c, cls in COLSUM_RUNS])
def test_colsum(hip, cuda, c, cls):
    op = gc.build_colsum(c, cls)
    M, N, n_w = c['M'], c['N'], c['n_w']
    Xw = gc.place(op['X'], c['mode']).to(cuda)
    X = gc.view_of(Xw, M, N, c['mode'])
    w = None
    if n_w:
        w = gc.view_of(gc.place(op['w'], 'ok').to(cuda), M, n_w, 'ok')
    n_out = max(n_w, 1) * N
    whole = (gc.nan_bits(n_out + 16) if op['base'] is None else gc.place_vec(op['base'].reshape(-1))).to(cuda)
    out = gc.vec_of(whole, n_out).view(op['shape'])
    pl = hip.colsum_plan(X, n_w)
    res = hip.colsum(X, out=out, accumulate=c['accumulate'], row_weight=w)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr() and gc.vec_guards_intact(whole, n_out)
    truth = gc.colsum_def(op['X'], op['w'], op['base'], torch.float64)
    if cls == 'int' or M == 0:
        gc.check_int(c['id'], out, truth)       # M = 0: zeros, or the prior content unchanged
    else:
        ref = gc.colsum_def(op['X'], op['w'], op['base'], torch.float32)
        record('colsum_partial%s_kernel<%d>' % ('_vec' if pl.vec else '', n_w), c['id'], *gc.check_real(c['id'], out, ref, truth, gc.RTOL))
