"""What tests/test_gemm_gpu.py rests on, checked without a GPU: the case tables of tests/gemm_cases.py reach every instantiation
and branch of the GEMM family -- asked of the library itself through the host-only plan queries psn_gemm_plan,
psn_gemm_tn_plan and psn_colsum_plan, the functions the launchers call --, the 'int' cases are exact in fp32, the float32
evaluation of every 'real' case stays within half the bound of the float64 one (so that helpers.assert_vs_truth allows the
kernel no element beyond the bound), and six wrong formulations of the definitions fail the very checks the GPU test applies."""
import collections
import itertools
import os

import pytest
import torch

from tests import gemm_cases as gc

LAYOUT_NAME = {(False, True): 'NT', (False, False): 'NN', (True, False): 'TN', (True, True): 'TT'}


@pytest.fixture(scope='module')
def hip():
    from psnerf_amd import hip
    return hip


def test_epilogue_codes_equal_the_header():
    from psnerf_amd import cabi
    consts = cabi.parse(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'psnerf_hip.h'))[0]
    assert {k[len('PSN_EPI_'):]: v for k, v in consts.items() if k.startswith('PSN_EPI_')} == gc.EPI
    assert consts['PSN_GEMM_TN_MAX_ITEMS'] == 12 == len(gc.tn_chunks(list(range(13)))[0])


def test_family_a_covers_every_pair():
    shapes = {(c['M'], c['N'], c['K']) for c in gc.GEMM_CASES if c['family'] == 'A' and 'pair' in c['id']}
    for layout in gc.LAYOUTS:
        assert {(c['M'], c['N'], c['K']) for c in gc.GEMM_CASES if c['family'] == 'A' and 'pair' in c['id'] and (c['ta'], c['tb']) == layout} == shapes
    for (i, xs), (j, ys) in itertools.combinations(enumerate((gc.A_M, gc.A_N, gc.A_K)), 2):
        assert {(s[i], s[j]) for s in shapes} == set(itertools.product(xs, ys)), 'pairs of dimensions %d, %d' % (i, j)


# --------------------------------------------------------------------------- coverage, as the library's own dispatcher sees it
def tn256_regimes(nt):
    """The loops of gemm_tn256_grouped_kernel a slice of ``nt`` k-tiles enters: mask-free steady pairs (steps <= nt - 3), masked
    pairs, the single masked tail."""
    steady = len(range(0, max(nt - 3, 0), 2))
    rest = nt - 2 * steady
    return (['steady'] if steady else []) + (['pair'] if rest >= 2 else []) + (['tail'] if nt % 2 else [])


def reached(hip):
    """{what is reached: set of the ids of the cases that reach it}."""
    hit = collections.defaultdict(set)
    for c in gc.GEMM_CASES:
        pl = gc.gemm_plan_of(c)
        nt = {128: 2, 256: 4}[pl.bn]
        mark = lambda key: hit[key].add(c['id'])
        mark('gemm_kernel<%s,%d>' % (LAYOUT_NAME[(c['ta'], c['tb'])], nt))
        mark('gemm a_vec=%d' % pl.a_vec)
        mark('gemm b_vec=%d' % pl.b_vec)
        mark('gemm c_vec=%d' % pl.c_vec)
        e = c['epi']
        if e != 'NONE':
            mark('epilogue %s NT=%d full4=%s' % (e, nt, 'none' if c['N'] <= 3 else ('ragged' if c['N'] % 4 else 'all')))
            mark('epilogue %s c_vec=%d' % (e, pl.c_vec))
        if e in gc.NEED_AUX1:
            mark('epilogue %s auxin_vec=%d' % (e, pl.auxin_vec))
        if e in gc.NEED_AUX2:
            mark('epilogue %s auxin2_vec=%d' % (e, pl.auxin2_vec))
        if e in gc.NEED_AUXOUT or (e == 'BIAS_SOFTPLUS' and c['aux_out']):
            mark('epilogue %s auxout_vec=%d' % (e, pl.auxout_vec))
        if e == 'BIAS_SOFTPLUS' and not c['aux_out']:
            mark('epilogue BIAS_SOFTPLUS without aux_out')
        if pl.reduce:
            mark('splitk_reduce%s_kernel accumulate=%d' % ('_vec' if pl.reduce == 2 else '', e == 'ACCUM'))
            mark('split-K last slice of %d rows' % (c['K'] - (pl.split_k - 1) * pl.k_chunk))
            assert pl.k_chunk == c['k_chunk'], c['id']
            if pl.split_k < c['split_k']:
                mark('split-K fewer slices than requested')
            if nt == 4:
                mark('gemm_kernel<TN,4> through split-K, M=%d' % c['M'])
        elif c['split_k'] > 1:
            mark('split-K request collapses to one slice%s%s' % (' ACCUM' if e == 'ACCUM' else '', ' colsum' if c['colsum'] else ''))
    for c in gc.TN_CASES:
        items = gc.build_tn(c, None)
        for chunk in gc.tn_chunks(items):
            pl = hip.gemm_tn_plan(chunk, c['split_k'])
            for i, it in enumerate(chunk):
                mark = lambda key: hit[key].add(c['id'])
                kind = pl.kind[i]
                # the Python copies of the rule that size the workspace agree with the library
                assert hip._tn_is_big(it) == (kind == hip.TN_BIG) and hip._tn_is_tall(it) == (kind == hip.TN_TALL), c['id']
                nts = ([pl.nt[i]] if pl.live_slices[i] > 1 else []) + [pl.nt_last[i]]
                if kind == hip.TN_BIG:
                    form = 'DMA' if pl.dma[i] else 'staged'
                    mark('gemm_tn256_grouped_kernel %s' % form)
                    if c['x3']:
                        mark('gemm_tn256_x3_grouped_kernel')
                    for r in tn256_regimes(pl.nt_last[i]):
                        mark('tn256 %s %s, last tile of %s rows' % (form, r, {32: 32, 1: 1, 31: 31}.get(pl.last_tile_rows[i], 'other')))
                    for nt in nts:
                        mark('tn256 %s nt=%s' % (form, nt if nt <= 7 else '>7'))
                    if pl.live_slices[i] > 1:
                        mark('tn256 %s several slices, short last one' % form)
                elif kind == hip.TN_TALL:
                    mark('gemm_tn_tall_grouped_kernel')
                    for nt in nts:
                        mark('tall nt %s' % ('odd' if nt % 2 else 'even'))
                        if nt <= 3:
                            mark('tall nt=%d' % nt)
                    if pl.live_slices[i] > 1:
                        mark('tall several slices')
                else:
                    mark('gemm_tn_grouped_kernel')
                    mark('tile a_vec=%d' % pl.a_vec[i])
                    mark('tile b_vec=%d' % pl.b_vec[i])
                    if it['spec']['M'] > 128 and not it.get('b_div'):
                        mark('tile: fallback of a misaligned %s item' % ('256 x 256' if it['spec']['N'] > 128 else 'tall'))
                    if it.get('b_div'):
                        mark('table %s' % ('two tables' if it.get('B_tab2') is not None else 'one table'))
                        mark('table modulo %s' % ('wraps' if pl.b_mod[i] else 'cannot wrap'))
                        if pl.index_path[i] & hip.TN_INDEX_FAST:
                            mark('table index by fastdiv24')
                        if pl.index_path[i] & hip.TN_INDEX_DIV:
                            mark('table index by integer division')
                mark('grouped_reduce_kernel vec=%d accumulate=%d' % (pl.reduce_vec[i], it['accumulate']))
                if it['spec']['two']:
                    mark('two products, kind %d' % kind)
                if it['spec']['rows'] is not None:
                    mark('k_rows prefix, kind %d' % kind)
                if it['colsum']:
                    mark('column sums, kind %d' % kind)
        if len(items) > 12:
            hit['group of %d launches' % len(gc.tn_chunks(items))].add(c['id'])
    for c in gc.COLSUM_CASES:
        X = gc.view_of(torch.empty(gc.layout(c['M'], c['N'], c['mode'])[:2]), c['M'], c['N'], c['mode'])
        pl = hip.colsum_plan(X, c['n_w'])
        hit['colsum_partial%s_kernel<%d>' % ('_vec' if pl.vec else '', c['n_w'])].add(c['id'])
        hit['colsum N %s 256' % ('<=' if c['N'] <= 256 else '>')].add(c['id'])
        if c['M'] == 0:
            hit['colsum M=0 accumulate=%d' % c['accumulate']].add(c['id'])
        if pl.nblocks == 2048 // max(c['n_w'], 1) and c['M'] > 128 * pl.nblocks:
            hit['colsum nblocks at its cap'].add(c['id'])
        hit['colsum accumulate=%d' % c['accumulate']].add(c['id'])
    return hit


# Everything the suite has to reach.  A kernel variant added later is added here and fails until a case reaches it.
REQUIRED = (
    ['gemm_kernel<%s,%d>' % (l, nt) for l in LAYOUT_NAME.values() for nt in (2, 4)]
    + ['gemm %s_vec=%d' % (o, v) for o in 'abc' for v in (0, 1)]
    + ['epilogue %s NT=%d full4=%s' % (e, nt, f) for e in gc.EPI if e != 'NONE' for nt, fs in ((2, ('all', 'ragged', 'none')), (4, ('all', 'ragged')))
       for f in fs]
    + ['epilogue %s c_vec=%d' % (e, v) for e in gc.EPI if e != 'NONE' for v in (0, 1)]
    + ['epilogue %s auxin_vec=%d' % (e, v) for e in gc.NEED_AUX1 for v in (0, 1)]
    + ['epilogue %s auxin2_vec=%d' % (e, v) for e in gc.NEED_AUX2 for v in (0, 1)]
    + ['epilogue %s auxout_vec=%d' % (e, v) for e in gc.NEED_AUXOUT + ('BIAS_SOFTPLUS',) for v in (0, 1)]
    + ['epilogue BIAS_SOFTPLUS without aux_out']
    + ['splitk_reduce%s_kernel accumulate=%d' % (k, a) for k in ('', '_vec') for a in (0, 1)]
    + ['split-K last slice of %d rows' % r for r in (1, 15, 16)]
    + ['split-K fewer slices than requested', 'split-K request collapses to one slice ACCUM colsum']
    + ['gemm_kernel<TN,4> through split-K, M=%d' % m for m in (130, 256)]
    + ['gemm_tn_grouped_kernel', 'gemm_tn256_grouped_kernel DMA', 'gemm_tn256_grouped_kernel staged', 'gemm_tn256_x3_grouped_kernel',
       'gemm_tn_tall_grouped_kernel']
    + ['tn256 %s %s, last tile of %d rows' % (f, r, n) for f in ('DMA', 'staged') for r in ('steady', 'pair', 'tail') for n in (32, 1, 31)]
    + ['tn256 %s nt=%d' % (f, n) for f in ('DMA', 'staged') for n in range(1, 8)]
    + ['tn256 %s several slices, short last one' % f for f in ('DMA', 'staged')]
    + ['tall nt odd', 'tall nt even', 'tall nt=1', 'tall nt=2', 'tall nt=3', 'tall several slices']
    + ['tile %s_vec=%d' % (o, v) for o in 'ab' for v in (0, 1)]
    + ['tile: fallback of a misaligned 256 x 256 item', 'tile: fallback of a misaligned tall item']
    + ['table one table', 'table two tables', 'table modulo wraps', 'table modulo cannot wrap', 'table index by fastdiv24',
       'table index by integer division']
    + ['grouped_reduce_kernel vec=%d accumulate=%d' % (v, a) for v in (0, 1) for a in (0, 1)]
    + ['%s, kind %d' % (w, k) for w in ('two products', 'k_rows prefix', 'column sums') for k in (0, 1, 2)]
    + ['group of 2 launches', 'group of 3 launches']
    + ['colsum_partial%s_kernel<%d>' % (k, n) for k in ('', '_vec') for n in gc.H_NW]
    + ['colsum N <= 256', 'colsum N > 256', 'colsum M=0 accumulate=0', 'colsum M=0 accumulate=1', 'colsum nblocks at its cap',
       'colsum accumulate=0', 'colsum accumulate=1'])


@pytest.fixture(scope='module')
def hit(hip):
    return reached(hip)


def test_every_instantiation_and_branch_is_reached(hit):
    missing = [k for k in REQUIRED if not hit.get(k)]
    assert not missing, 'reached by no case: %s' % missing
    print('\n==== GEMM family: what the cases reach (number of cases, first case) ====')
    for k in REQUIRED:
        print('%-62s %4d  %s' % (k, len(hit[k]), sorted(hit[k])[0]))


def test_every_family_is_needed(hit):
    """Without any one of the families A - H something required is reached by no case."""
    fam = {c['id']: c['family'] for c in gc.ALL_CASES}
    for f in 'ABCDEFGH':
        only = [k for k in REQUIRED if {fam[i] for i in hit[k]} == {f}]
        assert only, 'family %s could go unnoticed' % f


# --------------------------------------------------------------------------- the 'int' class is exact
def test_int_cases_stay_below_2_24():
    """Entries in [-4, 4]: K * 16 (times one factor of 4 or two products, plus one addend) < 2^24; the {-1, 0, 1} cases:
    at most 2^24 nonzero terms of magnitude 1."""
    for c in gc.GEMM_CASES:
        if 'int' in c['classes']:
            assert c['epi'] in gc.EPI_EXACT and gc.gemm_int_bound(c) < gc.INT_LIMIT, c['id']
    for c in gc.TN_CASES:
        assert 'int' in c['classes']
        if c['hi'] == 1:
            assert c['lo'] == -1 and gc.tn_int_bound(c) <= gc.INT_LIMIT and c['classes'] == ('int',), c['id']
        else:
            assert (c['lo'], c['hi']) == (-4, 4) and gc.tn_int_bound(c) < gc.INT_LIMIT, c['id']
    for c in gc.COLSUM_CASES:
        assert gc.colsum_int_bound(c) < gc.INT_LIMIT, c['id']
    assert {c['K'] for c in gc.TN_CASES if c['hi'] == 1} == set(gc.FASTDIV_K)


def test_int_definition_is_exact_in_float32():
    """On 'int' operands the float32 evaluation of the definition equals the float64 one: a sample of each kind."""
    for c in [c for c in gc.GEMM_CASES if 'int' in c['classes'] and c['M'] < 1000][::9]:
        op = gc.build_gemm(c, 'int')
        for x, y in zip(gc.gemm_def(op, torch.float32), gc.gemm_def(op, torch.float64)):
            assert (x is None) == (y is None) and (x is None or torch.equal(x.double(), y)), c['id']
    for c in [c for c in gc.TN_CASES if c['K'] < 10000][::7]:
        for it in gc.build_tn(c, 'int'):
            for x, y in zip(gc.tn_item_def(it, c['K'], torch.float32), gc.tn_item_def(it, c['K'], torch.float64)):
                assert (x is None) == (y is None) and (x is None or torch.equal(x.double(), y)), c['id']


# --------------------------------------------------------------------------- the 'real' class: the reference within half the bound
def _ratio(ref, truth, rtol, tmax):
    """worst |ref - truth| / (rtol |truth| + rtol max|truth|), the bound of assert_vs_truth(rtol, 'max')."""
    if truth.numel() == 0:
        return 0.0
    return float(((ref.double() - truth).abs() / (rtol * truth.abs() + rtol * tmax)).max())


_WORST_REF = collections.defaultdict(float)


@pytest.mark.parametrize('c', [c for c in gc.GEMM_CASES if 'real' in c['classes']], ids=gc.case_id)
def test_real_reference_within_half_the_bound_gemm(c):
    op = gc.build_gemm(c, 'real')
    outs = gc.gemm_outputs(c)
    blocks = gc.row_blocks(c['M'])
    if len(blocks) == 1:
        truth, ref = gc.gemm_def(op, torch.float64), gc.gemm_def(op, torch.float32)
        worst = {name: _ratio(ref[i], truth[i], rtol, float(truth[i].abs().max())) for name, i, rtol in outs}
    else:       # block by block: the maximum of the truth first, the ratios after it
        tmax = collections.defaultdict(float)
        for rows in blocks:
            truth = gc.gemm_def(op, torch.float64, rows)
            for name, i, _ in outs:
                tmax[name] = max(tmax[name], float(truth[i].abs().max()))
        worst = collections.defaultdict(float)
        for rows in blocks:
            truth, ref = gc.gemm_def(op, torch.float64, rows), gc.gemm_def(op, torch.float32, rows)
            for name, i, rtol in outs:
                worst[name] = max(worst[name], _ratio(ref[i], truth[i], rtol, tmax[name]))
    for name, i, rtol in outs:
        key = gc.outputs_of(c['epi'], c['aux_out'])[i] if i < 2 else None
        _WORST_REF[key or 'linear'] = max(_WORST_REF[key or 'linear'], worst[name])
        assert worst[name] < 0.5, '%s %s: the float32 definition is %.3f of the bound from the float64 one' % (c['id'], name, worst[name])


@pytest.mark.parametrize('c', [c for c in gc.TN_CASES if 'real' in c['classes']], ids=gc.case_id)
def test_real_reference_within_half_the_bound_grouped(c):
    for n, it in enumerate(gc.build_tn(c, 'real')):
        truth, ref = gc.tn_item_def(it, c['K'], torch.float64), gc.tn_item_def(it, c['K'], torch.float32)
        for x, y in zip(ref, truth):
            if y is not None:
                w = _ratio(x, y, gc.RTOL, float(y.abs().max()))
                _WORST_REF['linear'] = max(_WORST_REF['linear'], w)
                assert w < 0.5, '%s item %d: %.3f of the bound' % (c['id'], n, w)


@pytest.mark.parametrize('c', gc.COLSUM_CASES, ids=gc.case_id)
def test_real_reference_within_half_the_bound_colsum(c):
    op = gc.build_colsum(c, 'real')
    truth, ref = gc.colsum_def(op['X'], op['w'], op['base'], torch.float64), gc.colsum_def(op['X'], op['w'], op['base'], torch.float32)
    if truth.numel() and float(truth.abs().max()) > 0:
        w = _ratio(ref, truth, gc.RTOL, float(truth.abs().max()))
        _WORST_REF['linear'] = max(_WORST_REF['linear'], w)
        assert w < 0.5, '%s: %.3f of the bound' % (c['id'], w)
    else:
        assert torch.equal(ref.double(), truth)


def test_report_reference_ratios():
    """(a record, printed with -s) worst ratio of the float32 definition per output class, in units of its bound."""
    print('\n==== float32 CPU definition vs float64, worst ratio in units of the bound ====')
    for k, v in sorted(_WORST_REF.items()):
        print('%-14s %.3f' % (k, v))


# --------------------------------------------------------------------------- seeded faults fail the checks of the GPU test
def _gemm_case(pred):
    return next(c for c in gc.GEMM_CASES if pred(c))


def _both_checks_fail(name, truth, ref, wrong64, wrong32, rtol=gc.RTOL):
    """``wrong*`` = the wrongly stated definition on 'int' (float64) and on 'real' operands (float32), standing in for the
    kernel: check_int and check_real must reject them, and accept the right definition."""
    t_int, t_real = truth
    gc.check_int(name, t_int.float(), t_int)
    gc.check_real(name, ref, ref, t_real, rtol)
    with pytest.raises(AssertionError):
        gc.check_int(name, wrong64.float(), t_int)
    with pytest.raises(AssertionError):
        gc.check_real(name, wrong32, ref, t_real, rtol)


def _gemm_fault(c, fault, out=0):
    oi, orr = gc.build_gemm(c, 'int'), gc.build_gemm(c, 'real')
    _both_checks_fail('%s %s' % (c['id'], fault), (gc.gemm_def(oi, torch.float64)[out], gc.gemm_def(orr, torch.float64)[out]),
                      gc.gemm_def(orr, torch.float32)[out], gc.gemm_def(oi, torch.float64, fault=fault)[out],
                      gc.gemm_def(orr, torch.float32, fault=fault)[out])


def test_fault_k_row_dropped_at_a_slice_seam():
    _gemm_fault(_gemm_case(lambda c: c['family'] == 'D' and c['K'] == 33 and c['epi'] == 'NONE'), 'drop_seam')
    _gemm_fault(_gemm_case(lambda c: c['family'] == 'B' and c['split_k'] > 1 and c['epi'] == 'ACCUM'), 'drop_seam')


def test_fault_last_row_duplicated():
    """The prefetch clamp without its mask: the tile after the last one re-reads the last row."""
    for fam, K in (('E', 33), ('E', 513), ('F', 193)):
        c = next(c for c in gc.TN_CASES if c['family'] == fam and c['K'] == K)
        ii, ir = gc.build_tn(c, 'int'), gc.build_tn(c, 'real')
        for n in range(len(ii)):
            d = lambda it, dt, f=None: gc.tn_item_def(it, c['K'], dt, fault=f)[0]
            _both_checks_fail('%s item %d' % (c['id'], n), (d(ii[n], torch.float64), d(ir[n], torch.float64)), d(ir[n], torch.float32),
                              d(ii[n], torch.float64, 'dup_last'), d(ir[n], torch.float32, 'dup_last'))


def test_fault_column_group_shifted_by_four():
    _gemm_fault(_gemm_case(lambda c: c['family'] == 'A' and c['N'] == 130 and c['K'] == 33), 'col_shift')
    _gemm_fault(_gemm_case(lambda c: c['family'] == 'C' and c['N'] == 217 and c['epi'] == 'MUL2'), 'col_shift', out=1)


def test_fault_bias_of_the_next_column():
    _gemm_fault(_gemm_case(lambda c: c['family'] == 'C' and c['N'] == 217 and c['epi'] == 'BIAS'), 'bias_shift')
    _gemm_fault(_gemm_case(lambda c: c['family'] == 'C' and c['N'] == 3 and c['epi'] == 'BIAS_RELU'), 'bias_shift')


def test_fault_mul_pos_with_greater_or_equal():
    _gemm_fault(_gemm_case(lambda c: c['family'] == 'C' and c['N'] == 217 and c['epi'] == 'MUL_POS'), 'pos_ge')


def test_fault_table_row_off_by_one_at_a_multiple_of_the_divisor():
    c = next(c for c in gc.TN_CASES if c['id'].startswith('G-table'))
    ii, ir = gc.build_tn(c, 'int'), gc.build_tn(c, 'real')
    n_tab = 0
    for n in range(len(ii)):
        if ii[n].get('b_div', 0) > 1 or ii[n].get('b2_div', 0) > 1:
            n_tab += 1
            d = lambda it, dt, f=None: gc.tn_item_def(it, c['K'], dt, fault=f)[0]
            _both_checks_fail('%s item %d' % (c['id'], n), (d(ii[n], torch.float64), d(ir[n], torch.float64)), d(ir[n], torch.float32),
                              d(ii[n], torch.float64, 'div_off'), d(ir[n], torch.float32, 'div_off'))
    assert n_tab >= 4
