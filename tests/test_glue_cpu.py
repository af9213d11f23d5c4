"""The cases and definitions of tests/glue_cases.py, checked without a GPU: every launch path that ``*_path`` can name is reached
by some case (the tables are written out below), every fp32 restatement stays within the caps that keep the GPU test's measured
allowance from hiding a failure (at most 2 % of its elements beyond half the bound, worst element at most 4 x the bound; the
measured figures are printed), deliberately wrong formulations fail the GPU test's own comparators, and the entry points refuse
bad arguments through the C ABI with a message that names them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import glue_cases as gc

F32, F64 = gc.F32, gc.F64


@pytest.fixture(autouse=True)
def _caps_on():
    gc.CAPS = True
    yield
    gc.CAPS = False


def _print_caps(title, prefix):
    print('\n%s: fp32 restatement vs float64 -- worst share beyond half the bound, worst |error| / bound' % title)
    for k, (share, worst) in sorted(gc._CAPS.items()):
        if k.startswith(prefix):
            print('  %-16s %5.2f %%  %5.2f' % (k, 100 * share, worst))


# ----------------------------------------------------------------------------------------------------------- path coverage
def test_every_path_is_covered():
    have = {}
    add = lambda fam, path, c: have.setdefault((fam, path), []).append(c)
    pe_all = gc.PE_ENC_CASES + gc.PE_ENC_CAP_CASES + gc.PE_JVP_CASES + gc.PE_JVP_CAP_CASES + gc.PE_BWD_CASES + gc.PE_BWD_CAP_CASES + gc.APP_CASES + gc.APP_CAP_CASES
    for c in pe_all:
        add('pe', gc.pe_path(c), c)
    need_pe = [('enc_generic', 1), ('enc64', 1), ('enc_generic_from64', 1), ('enc_generic', 2), ('enc_generic', 3), ('enc64', 2),
               ('enc_generic_from64', 5), ('jvp_generic', 1), ('jvp64', 1), ('jvp_generic_from64', 1), ('jvp_generic', 2), ('jvp64', 2),
               ('jvp_generic_from64', 5), ('bwd', 1), ('bwd', 2), ('app', 1), ('app', 2)]
    for path in need_pe:
        assert ('pe', path) in have, 'no case reaches %s, pass %d' % path
    # the first row of pass 2 is the issue's arithmetic: 53 774 rows (stride 39), 131 073 (four columns per thread), 699 051 (backward)
    assert gc.PASS // 39 + 1 == 53774 and gc.PASS // 16 + 1 == 131073 and gc.PASS // 3 + 1 == 699051
    for c in gc.PE_ENC_CAP_CASES + gc.PE_JVP_CAP_CASES + gc.PE_BWD_CAP_CASES + gc.APP_CAP_CASES:
        rows = gc.pe_pass_rows(c)
        assert len(rows) >= 2 and rows[-1][2] == c['n'] and all(b > a for _, a, b in rows), c['id']
    # every n_freqs at every stride; every n and every scale on each of the three encode paths; |x| <= 50 at 16 bands; special rows
    for nf in gc.PE_FREQS:
        w = gc.pe_width(nf)
        want = {w, w + 1, 100} | ({64} if w <= 64 else set())
        assert {c['stride'] for c in gc.PE_ENC_CASES if c['nf'] == nf} >= want, nf
        assert {c['scale'] for c in gc.PE_BWD_CASES if c['nf'] == nf} == set(gc.PE_SCALES)
    for kernel in ('enc_generic', 'enc64', 'enc_generic_from64'):
        cs = have[('pe', (kernel, 1))]
        assert {c['n'] for c in cs} == set(gc.PE_N) and {c['scale'] for c in cs} == set(gc.PE_SCALES), kernel
        assert {(c['n'], c['scale']) for c in cs if c['nf'] == 6} >= {(n, s) for n in gc.PE_N for s in gc.PE_SCALES}
    assert any(c['lim'] == 50.0 and c['nf'] == 16 for c in gc.PE_ENC_CASES) and any(c['lim'] == 1.0 and c['nf'] == 16 for c in gc.PE_ENC_CASES)
    assert any(len(gc.pe_inputs(c)['special']) == 6 for c in gc.PE_ENC_CASES)
    assert {(c['n'], c['form']) for c in gc.PE_BWD_CASES} >= {(n, f) for n in gc.PE_BWD_N for f in gc.PE_BWD_FORMS}
    assert 85 * 3 < 256 < 86 * 3
    assert {(c['nf'], c['n']) for c in gc.APP_CASES + gc.APP_CAP_CASES} >= {(nf, q) for nf in gc.APP_FREQS for q in gc.APP_Q} | {(4, 131073)}

    # weight norm
    wn = set().union(*[gc.wn_path(c) for c in gc.WN_CASES])
    need_wn = {'scale==1', 'scale!=1', 'cols<64', 'cols==64', 'cols>64', 'lane iterations 1', 'lane iterations 2',
               'lane iterations 5', 'item boundary inside a block', 'items in one block: 4', 'items in one block: 2', 'last block partly idle',
               '16 items in a launch', '1 items in a launch', 'launches 1', 'launches 2'}
    assert need_wn <= wn, need_wn - wn
    for kind, want in (('rand', set(gc.WN_WIDTHS)), ('exact', set(gc.WN_WIDTHS))):
        assert {it['cols'] for c in gc.WN_CASES for it in c['items'] if it['kind'] == kind} >= want
    assert {it['rows'] for c in gc.WN_CASES for it in c['items']} >= set(gc.WN_ROWS)
    assert {it['norm'] for c in gc.WN_CASES for it in c['items']} == {1e-6, 1.0, 1e6}
    assert [it['rows'] for it in gc.WN_CASES[2]['items']] == [1, 1, 1, 1, 3, 2, 7]
    for it, (v, g, dw) in zip(gc.WN_CASES[6]['items'], gc.wn_inputs(gc.WN_CASES[6])):   # the exact cases are what they claim
        n2 = (v.astype(F64) ** 2).sum(1)
        assert np.array_equal(np.sqrt(n2), np.round(np.sqrt(n2))) and np.array_equal(np.log2(np.abs(g)), np.round(np.log2(np.abs(g))))
        assert np.log2(it['scale']) == round(np.log2(it['scale']))
        if it['cols'] > 64:
            assert (np.flatnonzero(np.abs(v).sum(0)) >= 64).any()
        if it['rows'] >= 4:
            assert ((dw.astype(F64) * v).sum(1) == 0).any() and ((dw.astype(F64) * v).sum(1) != 0).any()

    # light rows: LDS chunks 0 .. 3 x blocks 1 .. 3, every gradient pairing at three chunks; duplicates across both chunk boundaries
    lr = {gc.lr_path(c) for c in gc.LR_CASES}
    assert {(ch, bl) for ch, bl, _ in lr} == {(ch, bl) for ch in range(4) for bl in (1, 2, 3)}
    assert {m for ch, bl, m in lr if ch == 3 and bl == 3} == set(gc.LR_MODES) and {m for ch, _, m in lr if ch == 0} == set(gc.LR_MODES)
    c = [c for c in gc.LR_CASES if (c['n_idx'], c['n_rows']) == (513, 600)][0]
    inp = gc.lr_inputs(c)
    assert [int(inp['idx'][p]) for p in gc.LR_DUP_POS] == [inp['dup']] * 4 and (inp['idx'] == inp['dup']).sum() >= 4

    # mask count, surface index, inverse index, copies
    mc = {gc.mc_path(c) for c in gc.MC_CASES}
    assert mc >= {(w, t, b) for w in ('words', 'bytes') for t in ('tail', 'no tail') for b in ('b', 'no b')}
    assert {c['n'] for c in gc.MC_CASES} == set(gc.MC_N)
    assert {c['off'] for c in gc.MC_CASES if gc.mc_path(c)[0] == 'bytes'} >= {(0, 1), (1, 0), (1, None)}
    si = {gc.si_path(c) for c in gc.SI_CASES}
    for q in (0, 1, 2, 5):
        assert any(p[0] == 'bytes per thread %d' % q for p in si)
    assert {p[1] for p in si} == {'idle threads', 'all threads'} and {p[2] for p in si} == {'truncated', 'padded', 'exact fit'} and {p[3] for p in si} == {'empty', 'live'}
    assert ('bytes per thread 2', 'idle threads', 'truncated', 'live') in si and {c['n'] for c in gc.SI_CASES} == set(gc.SI_N)
    assert {(c['n_pix'], c['count'], c['pad']) for c in gc.II_CASES} == {(n, cn, pd) for n in gc.II_NPIX for cn in gc.II_COUNTS for pd in (False, True)}
    c2 = set().union(*[gc.c2_path(c) for c in gc.C2_CASES])
    assert c2 >= {'1-D', '2-D', 'elements < 256', 'elements == 256', 'elements > 256', 'ld_src > cols', 'ld_dst > cols', '16 items in a launch',
                  '17 items in a launch', '24 items in a launch', '1 items in a launch', 'launches 1', 'launches 2'}

    # view batch: every job kind, the light-direction loop at 0 / 1 / 2 iterations, both job numberings, every type x pixel source
    vb = {gc.vb_path(c) for c in gc.VB_CASES}
    assert {(p[0], p[1]) for p in vb} == {(t, s) for t in gc.VB_TYPES for s in ('list', 'pix0=0', 'pix0>0')}
    assert {p[2] for p in vb} >= {('attr',), ('attr', 'vtg'), ('attr', 'rgb'), ('attr', 'rgb', 'vis'), ('attr', 'rgb', 'vtg'), ('attr', 'rgb', 'vis', 'vtg')}
    assert {p[3] for p in vb} == {0, 1, 2} and {p[4] for p in vb} == {None, 'Lv=L', 'Lv=0'}
    for t in gc.VB_TYPES:
        assert {p[3] for p in vb if p[0] == t} >= {1, 2} and {p[4] for p in vb if p[0] == t} >= {'Lv=L', 'Lv=0'}
        assert {c['n'] for c in gc.VB_CASES if c['dtype'] == t} == set(gc.VB_N) and {c['L'] for c in gc.VB_CASES if c['dtype'] == t} == {0, 1, 4, 96}
    assert any(c['n'] == 1 and c['L'] == 96 for c in gc.VB_CASES)
    assert {c['drop'] for c in gc.VB_CASES} == set(gc.VB_OUTPUTS[1:]) | {None}
    assert len(set(gc.vb_indices(dict(n=5, L=4, view=0, pix='list', V=3))[0].tolist())) == 3   # lidx has a repeat

    print('\ncovered paths (family: path -> cases)')
    for (fam, path), cs in sorted(have.items(), key=str):
        print('  %-4s %-28s %d' % (fam, path, len(cs)))
    for fam, paths in (('wn', wn), ('lr', lr), ('mc', mc), ('si', si), ('c2', c2), ('vb', vb)):
        for p in sorted(paths, key=str):
            print('  %-4s %s' % (fam, p))
    counts = dict(pe_encode=len(gc.PE_ENC_CASES + gc.PE_ENC_CAP_CASES), pe_jvp=len(gc.PE_JVP_CASES + gc.PE_JVP_CAP_CASES),
                  pe_bwd=len(gc.PE_BWD_CASES + gc.PE_BWD_CAP_CASES), app_input=len(gc.APP_CASES + gc.APP_CAP_CASES), weight_norm=len(gc.WN_CASES),
                  normalize=len(gc.NORM_N) * len(gc.NORM_EPS), light_rows=len(gc.LR_CASES), camera_rays=len(gc.CAM_CASES), mask_count=len(gc.MC_CASES),
                  surface_index=len(gc.SI_CASES), inverse_index=len(gc.II_CASES), copy2d=len(gc.C2_CASES), view_batch=len(gc.VB_CASES))
    print('cases: %s = %d' % (counts, sum(counts.values())))


# ---------------------------------------------------------------------------------------------------------- restatements
def test_pe_restatements_within_caps():
    for c in gc.PE_ENC_CASES + gc.PE_JVP_CASES + gc.PE_BWD_CASES + gc.PE_ENC_CAP_CASES + gc.PE_JVP_CAP_CASES + gc.PE_BWD_CAP_CASES:
        inp = gc.pe_inputs(c)
        fn = gc.pe_bwd_values if c['kind'] == 'bwd' else gc.pe_encode_values
        gc.check_pe(c, inp, fn(inp, c, F32))
    for c in gc.APP_CASES + gc.APP_CAP_CASES:
        inp = gc.pe_inputs(c)
        gc.check_app(c, inp, gc.app_restatement(c, inp))
    _print_caps('pe.hip', ('pe_', 'app_'))


def _wn_outputs(case, inputs, variant=None):
    return [gc.wn_kernel32(it, *x) if it['kind'] == 'exact' and variant is None else gc.wn_torch32(it, *x, variant=variant) for it, x in zip(case['items'], inputs)]


def test_weight_norm_restatements_within_caps():
    for case in gc.WN_CASES:
        inputs = gc.wn_inputs(case)
        gc.check_wn(case, inputs, _wn_outputs(case, inputs))
        if case['id'] == 'zero row':   # NaN in that row only
            for it, o in zip(case['items'], _wn_outputs(case, inputs)):
                bad = {k: np.flatnonzero(~np.isfinite(o[k].reshape(it['rows'], -1)).all(1)).tolist() for k in ('w', 'dv', 'dg')}
                assert all(v == ([2] if it['kind'] == 'zero_row' else []) for v in bad.values()), bad
    _print_caps('weight_norm.hip', 'wn_')


def _wn_decade_ok(fn, nrm):
    """Whether a float32 formulation of the backward is finite and within the cap at row norm ``nrm`` on three widths."""
    case = dict(id='probe', items=[gc._it(5, w, gc.S2, 'rand', nrm) for w in (5, 64, 289)])
    try:
        for it, x in zip(case['items'], gc.wn_inputs(case)):
            o, t = fn(it, *x), gc.wn_truth(it, *x)
            for k in ('dv', 'dg'):
                if not np.isfinite(o[k]).all():
                    return False
                gc.ref_caps('probe', o[k], t[k], gc.RTOL_WN_BWD, gc.RTOL_WN_BWD * float(np.abs(t['dv_term']).max()) if k == 'dv' else 'max')
    except AssertionError:
        return False
    return True


def test_weight_norm_norm_range_is_the_recorded_one():
    """The decades of |v| over which the fp32 torch formulation of the backward, and the kernel's restatement (which cubes the
    norm), stay finite and within the backward bound: measured here, recorded in glue_cases, and the kernel's test norms lie inside."""
    for label, fn, rec in (('torch', gc.wn_torch32, gc.WN_TORCH_FINITE), ('kernel', gc.wn_kernel32, gc.WN_KERNEL_FINITE)):
        ok = [e for e in range(-30, 31) if _wn_decade_ok(fn, 10.0 ** e)]
        print('\n%s formulation: backward finite and within the cap for |v| = 1e%d .. 1e%d' % (label, ok[0], ok[-1]))
        assert ok == list(range(ok[0], ok[-1] + 1)) and (10.0 ** ok[0], 10.0 ** ok[-1]) == rec, (label, ok[0], ok[-1], rec)
    lo = max(gc.WN_TORCH_FINITE[0], gc.WN_KERNEL_FINITE[0])
    hi = min(gc.WN_TORCH_FINITE[1], gc.WN_KERNEL_FINITE[1])
    assert all(lo <= it['norm'] <= hi for c in gc.WN_CASES for it in c['items'])


def test_row_kernel_restatements_within_caps():
    for n in gc.NORM_N:
        for eps in gc.NORM_EPS:
            x, g = gc.norm_inputs(n, eps)
            gc.check_norm('n%d eps%g' % (n, eps), x, g, eps, gc.norm_fwd(x, eps, F32), gc.norm_bwd(x, g, eps, F32))
            nrm = gc._norm(x, F64)
            if n >= 255:   # more than one row on either side of the clamp, one exactly at it
                e = float(F32(eps))
                assert (nrm < e).sum() >= 4 and ((nrm >= e) & (nrm < 10 * e)).sum() >= 3 and (nrm == e).sum() == 1 and np.isinf(nrm).sum() == 1
    for c in gc.CAM_CASES:
        inp = gc.cam_inputs(c)
        gc.check('camera_rays: ' + c['id'], gc.cam_values(inp, c, F32), gc.cam_values(inp, c, F32), gc.cam_values(inp, c, F64), gc.RTOL_VALUE, gc.ATOL_UNIT)
    for c in gc.LR_CASES:
        inp = gc.lr_inputs(c)
        rows = inp['tab'][inp['idx']]
        gc.check('light_fwd: ' + c['id'], gc.norm_fwd(rows, 1e-12, F32), gc.norm_fwd(rows, 1e-12, F32), gc.norm_fwd(rows, 1e-12, F64), gc.RTOL_VALUE, gc.ATOL_UNIT)
        terms = gc.norm_bwd(rows, inp['g_dir'], 1e-12, F32)
        a, r, t = gc._row_scaled(terms, terms, gc.norm_bwd(rows, inp['g_dir'], 1e-12, F64))
        gc.check('light_bwd_terms: ' + c['id'], a, r, t, gc.RTOL_GRAD, gc.RTOL_GRAD)
        gc.check_lr_bwd(c, inp, terms, gc.lr_scatter_sum(inp['idx'], terms, c['n_rows']), gc.lr_scatter_sum(inp['idx'], inp['g_int'], c['n_rows']))
    _print_caps('small.hip', ('normalize_', 'camera_', 'light_'))


def test_index_and_gather_truths_are_what_they_say():
    """The exact truths against an independent formulation: torch.nonzero, a pixel loop, torch indexing."""
    for c in gc.SI_CASES:
        byt, cap = gc.si_inputs(c)
        idx, count = gc.si_truth(byt, cap)
        nz = torch.from_numpy(byt != 0).nonzero()[:, 0]
        live = min(cap, nz.numel())
        assert count == nz.numel() and idx[:live].tolist() == nz[:cap].tolist() and set(idx[live:].tolist()) <= {int(nz[-1]) if nz.numel() else 0}
    for c in gc.II_CASES:
        idx, count = gc.ii_inputs(c)
        inv = gc.ii_truth(idx, count, c['n_pix'])
        ns = idx.size if count is None else min(int(count), idx.size)
        for p in range(c['n_pix']):
            hits = [k for k in range(ns) if idx[k] == p]
            assert inv[p] == (hits[0] if hits else -1)
        if c['pad'] and c['count'] in ('none', 'above') and idx.size > 5:
            assert inv[idx[-1]] == idx.size - 6   # the padded repeats map to their first row
    for c in gc.MC_CASES[:12]:
        a, b = gc.mc_inputs(c)
        assert gc.mc_truth(a, b) == float((torch.from_numpy(a).bool() & (torch.from_numpy(b).bool() if b is not None else True)).sum())
    a, b = gc.mc_inputs(gc.MC_CASES[-1])
    assert set(np.unique(a)) == set(np.unique(b)) == {0, 1, 2, 0x7f, 0x80, 0xff}
    for c in gc.VB_CASES[::7]:
        t = gc.vb_tables(c['view'], c['dtype'])
        want = gc.vb_truth(c, t)
        lidx, pix, pix0, vidx = gc.vb_indices(c)
        px = torch.from_numpy(pix) if pix is not None else pix0 + torch.arange(c['n'])
        if 'rgb' in want:
            img = torch.from_numpy(t['images']) if c['dtype'] == 'float32' else torch.from_numpy(t['lut'])[torch.from_numpy(t['images'].astype(np.int64))]
            ref = (img[torch.from_numpy(lidx)] * torch.from_numpy(t['object_mask'])[None, :, None])[:, px]
            assert torch.equal(torch.from_numpy(want['rgb']), ref)
            assert bool((ref[:, ~torch.from_numpy(t['object_mask'])[px]] == 0).all())
        assert want['uv'].tolist() == [[float(k % gc.VB_W), float(k // gc.VB_W)] for k in px.tolist()]
        gc.check_vb(c, want, want)
    assert abs(float(gc.vb_tables(0, 'uint8')['lut'][255]) - 1.0) > 1e-3   # not k / 255


# ------------------------------------------------------------------------------------------------------ wrong formulations
def _enc(variant, c):
    inp = gc.pe_inputs(c)
    gc.check_pe(c, inp, gc.pe_encode_values(inp, c, F32, variant))


def _bwd(variant, c):
    inp = gc.pe_inputs(c)
    gc.check_pe(c, inp, gc.pe_bwd_values(inp, c, F32, variant))


def _app(variant, c):
    inp = gc.pe_inputs(c)
    gc.check_app(c, inp, gc.app_restatement(c, inp, variant))


def _wn(variant, case):
    inputs = gc.wn_inputs(case)
    gc.check_wn(case, inputs, _wn_outputs(case, inputs, variant))


def _norm_bwd(variant, n, eps):
    x, g = gc.norm_inputs(n, eps)
    gc.check_norm('n%d' % n, x, g, eps, None, gc.norm_bwd(x, g, eps, F32, variant))


def _lr(variant, c):
    inp = gc.lr_inputs(c)
    terms = gc.norm_bwd(inp['tab'][inp['idx']], inp['g_dir'], 1e-12, F32)
    gc.check_lr_bwd(c, inp, terms, gc.lr_scatter_sum(inp['idx'], terms, c['n_rows'], variant), gc.lr_scatter_sum(inp['idx'], inp['g_int'], c['n_rows'], variant))


def _ii(variant, c):
    idx, count = gc.ii_inputs(c)
    gc.check_equal(c['id'], gc.ii_truth(idx, count, c['n_pix'], variant), gc.ii_truth(idx, count, c['n_pix']))


def _cam(variant, c):
    inp = gc.cam_inputs(c)
    gc.check('camera_rays: ' + c['id'], gc.cam_values(inp, c, F32, variant), gc.cam_values(inp, c, F32), gc.cam_values(inp, c, F64), gc.RTOL_VALUE, gc.ATOL_UNIT)


def _vb(variant, c):
    t = gc.vb_tables(c['view'], c['dtype'])
    gc.check_vb(c, gc.vb_truth(c, t, variant), gc.vb_truth(c, t))


_ENC = [c for c in gc.PE_ENC_CASES + gc.PE_JVP_CASES if c['nf'] >= 1]
_BWD = [c for c in gc.PE_BWD_CASES if c['nf'] >= 1 and c['form'] != 'zero']
WRONG = {
    'encode: sin and cos swapped in one band': (_enc, 'swap', _ENC),
    'encode: the last band at 2^(f-1)': (_enc, 'last_band', _ENC),
    'encode: components permuted': (_enc, 'perm', _ENC),
    'app_input: sin and cos swapped in one band': (_app, 'swap', [c for c in gc.APP_CASES if c['nf']]),
    'pe backward without 2^f': (_bwd, 'no_pow', [c for c in _BWD if c['nf'] >= 4]),
    'pe backward without scale': (_bwd, 'no_scale', [c for c in _BWD if c['scale'] != 1.0]),
    'pe backward: components permuted': (_bwd, 'perm', _BWD),
    'weight norm: dg without scale': (_wn, 'dg_no_scale', [c for c in gc.WN_CASES if c['id'].startswith(('widths', 'row norms', '16', '17'))]),
    'weight norm: dv without the projection term': (_wn, 'dv_no_projection', [c for c in gc.WN_CASES if c['id'].startswith(('widths', 'row norms', '16', '17'))]),
    'normalize backward ignoring the clamp': (lambda v, a: _norm_bwd(v, *a), 'ignore_clamp', [(n, e) for n in gc.NORM_N[1:] for e in gc.NORM_EPS]),
    'light rows backward keeps the first duplicate only': (_lr, 'first_duplicate_only', [c for c in gc.LR_CASES if c['n_idx'] >= 255 and c['n_rows'] > 1]),
    'inverse index maps a padded repeat to its last row': (_ii, 'last_repeat', [c for c in gc.II_CASES if c['pad'] and c['count'] in ('none', 'above') and c['n_pix'] > 1]),
    'camera rays: principal point permuted': (_cam, 'perm', gc.CAM_CASES),
    'view batch: visibility read at row l': (_vb, 'vis_row_l', [c for c in gc.VB_CASES if c['vis'] and c['L'] >= 4 and c['drop'] != 'visibility']),
    'view batch: object mask left out': (_vb, 'no_mask', [c for c in gc.VB_CASES if c['L'] and c['n'] >= 255]),
}


@pytest.mark.parametrize('what', sorted(WRONG))
def test_wrong_formulation_is_rejected(what):
    """Each mistake, evaluated in float32 in place of the kernel, fails the comparator of the GPU test on EVERY case that can
    show it -- the evidence that the GPU test would fail on a kernel that is wrong in this way."""
    fn, variant, cases = WRONG[what]
    assert cases
    for c in cases:
        fn(None, c)   # the correct formulation passes
        with pytest.raises(AssertionError):
            fn(variant, c)
    print('\n%s: rejected on %d cases' % (what, len(cases)))


# --------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_through_the_c_abi():
    """Refused on the host, before any launch and without a device: error code -1 and a message that names the entry point."""
    from psnerf_amd import hip
    lib, p = hip._lib, ctypes.c_void_p(64)

    def refused(rc, word):
        msg = lib.psn_last_error()
        assert rc == hip.E_ARG == -1 and word in msg, (rc, msg)
    refused(lib.psn_pe_encode(p, 4, 17, 1.0, p, 200, None), b'pe_encode: n_freqs=17')
    refused(lib.psn_pe_encode(p, 4, 6, 1.0, p, 38, None), b'pe_encode: n_freqs=6 out_stride=38')
    refused(lib.psn_pe_encode_jvp(p, p, 4, 17, 1.0, p, 200, None), b'pe_encode_jvp: n_freqs=17')
    refused(lib.psn_pe_encode_jvp(p, p, 4, 6, 1.0, p, 38, None), b'pe_encode_jvp: n_freqs=6 out_stride=38')
    refused(lib.psn_pe_encode_bwd(p, p, 4, 17, 1.0, 200, None, 0, p, None), b'pe_encode_bwd: n_freqs=17')
    refused(lib.psn_pe_encode_bwd(p, p, 4, 6, 1.0, 38, None, 0, p, None), b'pe_encode_bwd: n_freqs=6 out_stride=38')
    refused(lib.psn_pe_encode_bwd(p, p, 4, 6, 1.0, 39, p, 38, p, None), b'pe_encode_bwd: out2_stride=38')
    refused(lib.psn_app_input(p, p, p, 4, 10, p, None), b'app_input: n_freqs=10')
    refused(lib.psn_app_input(p, p, p, 4, -1, p, None), b'app_input: n_freqs=-1')
    items = (hip.PsnWnItem * 17)()
    for it in items:
        it.v, it.g, it.w, it.rows, it.cols, it.scale = 64, 64, 64, 2, 3, 1.0
    for fn in (lib.psn_weight_norm_fwd, lib.psn_weight_norm_bwd):
        refused(fn(0, ctypes.addressof(items), None), b'weight_norm: n_items=0')
        refused(fn(17, ctypes.addressof(items), None), b'weight_norm: n_items=17')
    items[1].dw, items[1].dv, items[1].dg = 64, 64, 64
    refused(lib.psn_weight_norm_bwd(2, ctypes.addressof(items), None), b'weight_norm: item 0: missing gradient')
    items[0].w = None
    refused(lib.psn_weight_norm_fwd(1, ctypes.addressof(items), None), b'weight_norm: item 0: missing output')
    refused(lib.psn_light_rows_bwd(p, p, 4, 8, 1e-12, p, None, None, None, None), b'light_rows_bwd: gradient pairs')
    refused(lib.psn_light_rows_bwd(p, p, 4, 8, 1e-12, None, None, None, p, None), b'light_rows_bwd: gradient pairs')
    c2 = (hip.PsnCopy2dItem * 2)()
    for it in c2:
        it.src, it.dst, it.rows, it.cols, it.ld_src, it.ld_dst = 64, 64, 2, 8, 8, 8
    c2[1].ld_dst = 7
    refused(lib.psn_copy2d_group(2, ctypes.addressof(c2), None), b'copy2d_group: item 1')
    c2[1].ld_dst, c2[0].ld_src = 8, 7
    refused(lib.psn_copy2d_group(2, ctypes.addressof(c2), None), b'copy2d_group: item 0')
    refused(lib.psn_copy2d_group(hip.COPY2D_MAX + 1, ctypes.addressof(c2), None), b'copy2d_group: n_items=25')
    refused(lib.psn_mask_count(p, None, 2 ** 24, p, None), b'mask_count: bad arguments (n=16777216')
    refused(lib.psn_surface_index(p, 2 ** 24, 8, p, None, None), b'surface_index: bad arguments (n=16777216')
    refused(lib.psn_surface_index(p, 100, 0, p, None, None), b'surface_index: bad arguments (n=100 cap=0)')
