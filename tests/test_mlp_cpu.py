"""What tests/test_mlp_gpu.py rests on, checked without a GPU: the plain-torch definitions of tests/mlp_cases.py equal the oracle
networks, the case tables reach every instantiation and both states of every launch switch of the fp32 dispatcher, the float32
evaluation of every case stays within half the bound of the float64 one (so that helpers.assert_vs_truth allows the kernel no
element beyond the bound), and five wrong formulations of the definition fail that very check.  The same for the
root finder (family H): both of its instantiations are reached by every case with the grid of the form, the kernel table of the
source holds no fp32 row outside mlp_cases.INSTANTIATIONS, the brackets are genuine (d_l < d_h, f_l < 0 < f_h, confirmed in float64),
the float32 definition's own iterates pass trace_check within half the allowance with no unchecked pair (worst ratio 0.15 here,
0.20 on the device's host), and five wrong root finders fail it.  259 tests, 8 s."""
import copy

import numpy as np
import pytest
import torch

from tests import mlp_cases as mc
from tests.helpers import assert_vs_truth, stage1_state_dict, stage2_state_dict, truth_ratios
from psnerf_amd.synthetic import stage1_cfg


def test_definition_equals_oracle_visibility_mlp():
    """evaluate() on the layers of the stage-2 visibility net (bear_conf) == oracle.stage2.MLP, light-major pair rows."""
    from oracle import stage2 as o2
    conf = o2.bear_conf()
    net = o2.PSNetwork(conf)
    net.load_state_dict(stage2_state_dict(conf, seed=31))
    vn = net.visibility_net.double()
    g = torch.Generator().manual_seed(8)
    Ns, L = 37, 3
    x = torch.rand(Ns, 3, generator=g) * 1.2 - 0.6
    l = torch.nn.functional.normalize(torch.randn(L, 3, generator=g), dim=-1)
    ea, eb = o2.embed(x, 10), o2.embed(l, 10)
    with torch.no_grad():
        ref = vn(torch.cat([ea.tile(L, 1), eb.repeat_interleave(Ns, dim=0)], -1).double())
    ws = [m.weight.detach().float() for m in vn.linears]
    bs = [m.bias.detach().float() for m in vn.linears]
    for mode in ('init', 'kt'):
        mine = mc.net_from_relu_mlp(ws, bs, 63, 63, vn.skip_at[0], ea, eb, (1, Ns, Ns, L), Ns * L, mode=mode,
                                    out_act='sigmoid' if vn.final == 'sigmoid' else 'none')
        out = mc.evaluate(mine, torch.float64)['out']
        assert out.shape == ref.shape
        assert float((out - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_definition_equals_oracle_occupancy_network():
    """evaluate() on the layers of the stage-1 geometry network == oracle.stage1.NeuralNetwork: only_occupancy and infer_occ."""
    from oracle import stage1 as o1
    cfg = stage1_cfg('bunny')
    net = o1.NeuralNetwork(cfg)
    net.load_state_dict(stage1_state_dict(cfg, seed=11))
    p = torch.rand(50, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1
    ws = [getattr(net, 'lin%d' % l).weight().detach() for l in range(net.n_geo)]
    bs = [getattr(net, 'lin%d' % l).bias.detach() for l in range(net.n_geo)]
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        occ_ref = net64(p.double(), only_occupancy=True)
        logit_ref = net64.infer_occ(p.double())[:, :1]
    for out_act, ref in (('occ', occ_ref), ('none', logit_ref)):
        mine = mc.net_from_geo(ws, bs, net.skips, net.octaves_pe, p, 1.0 / net.rescale, out_act=out_act)
        assert mc.layer_shape(mine)[net.skips[0]][:2] == (2, 7)   # the skip layer reads 7 activation k-tiles + the encoding
        out = mc.evaluate(mine, torch.float64)['out']
        assert float((out - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_activation_codes_equal_the_header():
    from psnerf_amd import cabi
    import os
    consts = cabi.parse(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'psnerf_hip.h'))[0]
    names = dict(none='NONE', relu='RELU', softplus='SOFTPLUS100', relu_mask='RELU_MASK', mul_aux='MUL_AUX', mul2='MUL2',
                 softplus_bwd='SOFTPLUS_BWD', head='HEAD', relu_bits='RELU_BITS', mul_aux_a='MUL_AUX_A', mul2_a='MUL2_A',
                 softplus_bwd_a='SOFTPLUS_BWD_A')
    assert set(names) == set(mc.ACT)
    for k, v in mc.ACT.items():
        assert consts['PSN_ACT_' + names[k]] == v
    assert [consts['PSN_OUT_' + k.upper()] for k in ('none', 'sigmoid', 'occ')] == [mc.OUT[k] for k in ('none', 'sigmoid', 'occ')]
    assert consts['PSN_MLP_MAX_LAYERS'] == mc.MAX_LAYERS and consts['PSN_PACK_MAX_ITEMS'] == 24 == mc.PACK_GROUP_SIZES[1]


def _all_dispatches():
    res = []
    for c in mc.ALL_NET_CASES:
        net = mc.build(c)
        for order in c.get('orders', (None,)):
            for live in (c.get('live') or (None,)):
                res.append((c, order, live, mc.dispatch(c, net, point_major=order != 'row', live=live)))
    for c in mc.H_CASES:      # the root finder: both forms of every case
        net = mc.root_inputs(c)[0]
        for row_parallel in (False, True):
            res.append((c, None, None, mc.dispatch(c, net, row_parallel=row_parallel)))
    return res


DISPATCHES = _all_dispatches()


def test_case_ids_are_unique_and_small():
    ids = [c['id'] for c in mc.ALL_NET_CASES + mc.ARG_CASES + mc.PACK_ITEMS + mc.H_CASES + mc.H_ARG_CASES]
    assert len(ids) == len(set(ids))
    for c in mc.ALL_NET_CASES + mc.H_CASES:
        assert (c.get('capacity') or c['n']) <= 1300, c['id']


def test_every_instantiation_of_the_fp32_dispatcher_is_covered():
    """lean and chain x NMT 4 / 8 / 16, TRIM lean and chain, FROMA with and without TRIM, SRC 2 and SRC 3, and the root finder in
    both forms (SRC 4 = feature-parallel, SRC 1 = row-parallel): the fp32 rows of the engine's kernel table."""
    seen = {d['name'] for _, _, _, d in DISPATCHES}
    assert seen == set(mc.INSTANTIATIONS), (sorted(seen), sorted(set(mc.INSTANTIATIONS) - seen))
    assert len(mc.INSTANTIATIONS) == 14
    for c in mc.H_CASES:     # every H case reaches both, with the grid of its form
        fp, rp = mc.dispatch(c, row_parallel=False), mc.dispatch(c, row_parallel=True)
        assert (fp['name'], fp['blocks']) == ('lean/16/src4/trim', (c['n'] + 15) // 16), c['id']
        assert (rp['name'], rp['blocks']) == ('lean/16/src1/trim', (c['n'] + 63) // 64), c['id']


def test_kernel_table_of_the_source_has_no_fp32_row_outside_the_list():
    """PSN_MLP_KERNELS of csrc/mlp_infer.hip, read as text: every row with x3 = false, and the feature-parallel root finder behind
    it, is an entry of mc.INSTANTIATIONS, and the other way round."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'psnerf_amd', 'csrc', 'mlp_infer.hip')).read()
    table = src[src.index('#define PSN_MLP_KERNELS(K)'):src.index('struct InferKernel')]
    rows = re.findall(r'K\((true|false), (\d+), (\d), (true|false), (true|false), (true|false)\)', table)
    assert len(rows) == 21 and 'kInferKernels[] = {PSN_MLP_KERNELS(PSN_KERNEL_ROW){0, 16, kSrcRootFp, 1, 0, 0, psn::root_find_fp_kernel}}' in src
    assert 'constexpr int kSrcRootFp = %d;' % mc.SRC_ROOT in src
    names = {'lean/16/src%d/trim' % mc.SRC_ROOT}
    for chain, nmt, s, trim, from_a, x3 in rows:
        if x3 == 'false':
            names.add('%s/%s%s%s%s' % ('chain' if chain == 'true' else 'lean', nmt, '/src' + s if s != '0' else '',
                                       '/trim' if trim == 'true' else '', '/froma' if from_a == 'true' else ''))
    assert names == set(mc.INSTANTIATIONS), sorted(names ^ set(mc.INSTANTIATIONS))


def test_every_launch_switch_occurs_in_both_states():
    for key in ('chain', 'trim', 'from_a', 'pair', 'point_major', 'half_final', 'wide_final', 'blocks_straddle'):
        states = {d[key] for _, _, _, d in DISPATCHES}
        assert states == {False, True}, (key, states)
    assert {d['hid'] for _, _, _, d in DISPATCHES} == {2, 4, 8}
    # init-B row: through LDS, from memory because a block straddles two B rows, from memory because bias + init rows do not fit
    tbs = {d['tb'] for _, _, _, d in DISPATCHES}
    assert {'none', 'lds', 'mem-straddle', 'mixed', 'mem-size'} <= tbs, tbs
    by_id = {c['id']: d for c, o, _, d in DISPATCHES if o != 'row'}
    assert by_id['B-depth10']['tb'] == 'lds' and by_id['B-depth11']['tb'] == 'mem-size' and by_id['B-depth12']['tb'] == 'mem-size'
    # a pair row set takes the row order when asked to, and a padded one with a ragged tail in either order
    for c, order, live, d in DISPATCHES:
        if order == 'row':
            assert not d['point_major']
        if c['id'].startswith('E-') and c['id'].endswith('tail70'):
            assert not d['point_major'], c['id']
    assert any(d['point_major'] for c, _, live, d in DISPATCHES if c['id'].startswith('E-') and live is not None)
    # pair launches: fewer than 8 blocks, groups shorter than a block (no pair), straddling blocks, a grid rounded up to 8
    pairs = {c['id']: d for c, o, _, d in DISPATCHES if c['id'].startswith('C-pair') and o == 'point'}
    assert pairs['C-pair-P64-G2-init']['pair'] and not pairs['C-pair-P29-G4-init']['pair']
    assert pairs['C-pair-P100-G3-init']['blocks_straddle'] and pairs['C-pair-P65-G9-init']['pair']
    assert (65 * 9 + 63) // 64 == 10      # 10 blocks -> a grid of 16


@pytest.mark.parametrize('c', mc.ALL_NET_CASES, ids=mc.case_id)
def test_float32_definition_within_half_the_bound(c):
    """The input condition of the GPU suite: no element of the float32 CPU evaluation lies beyond half the bound, which makes
    assert_vs_truth's allowance zero elements and a worst ratio of at most 1."""
    net = mc.build(c)
    t64, t32 = mc.evaluate(net, torch.float64), mc.evaluate(net, torch.float32)
    for (name, t), (_, r) in zip(mc.checked_tensors(c, t64), mc.checked_tensors(c, t32)):
        if t.numel() == 0:
            continue
        assert torch.isfinite(t).all()
        _, r_ref, _, n_allowed, worst_allowed = truth_ratios(r.numpy(), r.numpy(), t.numpy(), mc.RTOL, 'max')
        assert n_allowed == 0 and worst_allowed == 1.0 and float(r_ref.max()) <= 0.5, (c['id'], name, float(r_ref.max()))


def _case(id_):
    return [c for c in mc.ALL_NET_CASES if c['id'] == id_][0]


@pytest.mark.parametrize('wrong,case_id', [('swap_ab', 'B-tiles3+1-kt-w256'), ('swap_ab', 'B-tiles1+3-init-w256'),
                                           ('no_a_div', 'C-a_div5-a_mod7'), ('no_a_div', 'C-pointmajor-rows'),
                                           ('drop_skip', 'B-rows65-w256'), ('drop_skip', 'G-rows65'),
                                           ('double_bias', 'B-tiles2+0-init-w256'), ('double_bias', 'C-pair-P64-G2-init'),
                                           ('occ_sign', 'B-out1-occ'), ('occ_sign', 'G-sweep-rays3-steps64')])
def test_wrong_formulations_fail_the_bound(wrong, case_id):
    c = _case(case_id)
    net = mc.build(c)
    t64, t32 = mc.evaluate(net, torch.float64), mc.evaluate(net, torch.float32)
    bad = mc.evaluate(net, torch.float32, wrong=wrong)
    # the right float32 evaluation passes ...
    assert_vs_truth(case_id, t32['out'].numpy(), t32['out'].numpy(), t64['out'].numpy(), mc.RTOL, 'max')
    # ... the wrong one does not
    with pytest.raises(AssertionError):
        assert_vs_truth(case_id + ' ' + wrong, bad['out'].numpy(), t32['out'].numpy(), t64['out'].numpy(), mc.RTOL, 'max')
    assert wrong in mc.WRONG_FORMS


@pytest.mark.parametrize('item', mc.PACK_ITEMS, ids=mc.case_id)
def test_pack_reference_is_a_permutation_of_the_zero_extended_block(item):
    """pack_reference places every element of W exactly once and zeros elsewhere; the first fragment is the documented one."""
    store, view = mc.pack_matrix(item)
    ref = mc.pack_reference(view.numpy(), item['n_mt'], item['k_tiles'], item['transpose'])
    W = view.numpy().T if item['transpose'] else view.numpy()
    assert W.shape == (item['rows'], item['cols'])
    assert ref.size == item['n_mt'] * item['k_tiles'] * 1024
    assert np.array_equal(np.sort(ref[ref != 0]), np.sort(W[W != 0].ravel()))
    # element [kt][e][mt16][lane][c] by the formula of the header comment, at a few scattered places
    rs = np.random.RandomState(0)
    r5 = ref.reshape(item['k_tiles'], 2, 2 * item['n_mt'], 64, 4)
    for _ in range(200):
        kt, e, mt, lane, cc = rs.randint(item['k_tiles']), rs.randint(2), rs.randint(2 * item['n_mt']), rs.randint(64), rs.randint(4)
        row, col = 16 * mt + (lane & 15), 32 * kt + 16 * e + 4 * (lane >> 4) + cc
        want = W[row, col] if (row < W.shape[0] and col < W.shape[1]) else 0.0
        assert r5[kt, e, mt, lane, cc] == want


def test_sign_words_and_dead_rows():
    d = np.zeros((2, 64), dtype=np.float32)
    d[0, 16 * 2 + 4 * 3 + 1] = 1.0          # mt 2, g 3, r 1 -> word 3, bit 9
    d[1, 16 * 3 + 4 * 0 + 3] = 2.0          # mt 3, g 0, r 3 -> word 0, bit 15
    w = mc.sign_words(d)
    assert w.dtype == np.int64 and w[0].tolist() == [0, 0, 0, 1 << 9] and w[1].tolist() == [1 << 15, 0, 0, 0]
    full = mc.sign_words(np.ones((1, 256), dtype=np.float32))
    assert (full.view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    c = dict(n=3 * 192 + 70, period=192, save_row0=3 * 192)
    assert mc.dead_rows(c, 0).sum() == 3 * 192 and mc.dead_rows(c, 1).sum() == 3 * 128 and mc.dead_rows(c, 64).sum() == 3 * 128
    assert mc.dead_rows(c, 65).sum() == 3 * 64 and mc.dead_rows(c, 129).sum() == 0 and mc.dead_rows(c, 197).sum() == 0
    assert not mc.dead_rows(c, 0)[3 * 192:].any()


# --------------------------------------------------------------------------- H: the root finder
def test_root_cases_cover_what_the_kernels_branch_on():
    """Rays around both workgroup sizes; depths 1 .. 5 and 11 (odd: the extra barrier of the feature-parallel form, even: none, 11 +
    the final layer = PSN_MLP_MAX_LAYERS); a layer of 10 stages (8 + the encoding), of 9 (7 + the encoding) and of 7 without an
    input block; all three activations, octaves, scales and both thresholds; degenerate and benign brackets."""
    H = mc.H_CASES
    assert {c['n'] for c in H} >= {1, 15, 16, 17, 63, 64, 65, 129} and max(c['n'] for c in H) <= 129
    assert {c['depth'] for c in H} == {1, 2, 3, 4, 5, 11} and max(c['depth'] for c in H) + 1 == mc.MAX_LAYERS
    assert {c['act'] for c in H} == {'softplus', 'relu', 'none'} and {c['octaves'] for c in H} == {0, 6, 10}
    assert {round(c['pe_scale'], 6) for c in H} == {1.0, 0.5, round(2.0 / 3.0, 6)} and {c['tau'] for c in H} == {0.5, 0.3}
    assert set(mc.H_N_ITER) == {0, 1, 2, 3, 8, 64} and mc.H_STEPWISE == 8 and mc.H_TRACE == 3
    stages, trim_parity = set(), set()
    for c in H:
        net, inp = mc.root_inputs(c)
        shapes = mc.layer_shape(net)
        assert shapes[0] == (2, 0, False) and shapes[-1] == (0, 8, False) and len(shapes) == c['depth'] + 1
        stages |= {(kin, kact) for kin, kact, _ in shapes[1:-1]}
        if (0, 7, False) in shapes[1:-1]:
            trim_parity.add(c['depth'] % 2)
        kinds = inp['kinds']
        assert c['n'] == 1 or kinds.count('benign') >= 1, c['id']
        assert c['n'] < 8 or kinds.count('benign') >= 2, c['id']
    assert stages == {(2, 8), (2, 7), (0, 7), (0, 8)} and trim_parity == {0, 1}
    assert sum(mc.root_inputs(c)[1]['kinds'].count('dd') for c in H) >= 5 and sum(mc.root_inputs(c)[1]['kinds'].count('ff') for c in H) >= 5
    assert [a['id'] for a in mc.H_ARG_CASES] == ['H-ARG-n_iter-1', 'H-ARG-n_iter65', 'H-ARG-out_act', 'H-ARG-n_out3', 'H-ARG-bf16x2',
                                                 'H-ARG-softplus-final', 'H-ARG-in_kt_a1']


@pytest.mark.parametrize('c', mc.H_CASES, ids=mc.case_id)
def test_root_brackets_are_genuine(c):
    """Crossing rays: d_l < d_h and f_l < 0 < f_h, and the float64 definition at the two bracket ends has those very signs; the other
    rays carry the benign (0, 1, -1, 1) or one of the two degenerate brackets."""
    net, inp = mc.root_inputs(c)
    x = inp['crossing']
    dl, dh, fl, fh = inp['bracket']
    assert int(x.sum()) == inp['kinds'].count('x') >= 1
    assert (dl[x] < dh[x]).all() and (fl[x] < 0).all() and (fh[x] > 0).all()
    tau = float(np.float32(c['tau']))
    for d, sign in ((dl, -1), (dh, 1)):
        p = torch.from_numpy(inp['origin'][x].astype(np.float64) + d[x, None].astype(np.float64) * inp['direction'][x])
        val = mc.evaluate(net, torch.float64, points=p.float())['out'].reshape(-1).numpy() - tau
        assert (np.sign(val) == sign).all()
    for i, k in enumerate(inp['kinds']):
        b = inp['bracket'][:, i]
        if k == 'benign':
            assert b.tolist() == [0.0, 1.0, -1.0, 1.0]
        elif k == 'dd':
            assert b[0] == b[1] and b[2] < 0 < b[3]
        elif k == 'ff':
            assert b[2] == b[3] and b[0] < b[1]
    D = mc.root_find_definition(net, inp, 2)
    ff = np.array([k == 'ff' for k in inp['kinds']])
    dd = np.array([k == 'dd' for k in inp['kinds']])
    assert np.isinf(D[0][ff]).all() and not np.isfinite(D[2][ff]).any() and (D[2][dd] == dl[dd]).all() and np.isfinite(D[2][~ff]).all()


@pytest.mark.parametrize('c', mc.H_CASES, ids=mc.case_id)
def test_root_float32_definition_within_half_the_allowance(c):
    """The input condition of the GPU suite's float64 check: the float32 CPU definition's own iterates pass trace_check with a worst
    ratio of at most 0.5 and no unchecked (ray, iterate) pair."""
    net, inp = mc.root_inputs(c)
    r = mc.trace_check(net, inp, mc.root_find_definition(net, inp, mc.H_TRACE))
    print('%s worst ratio %.3f at %s' % (c['id'], r['worst'], r['where']))
    assert r['first_equal'] and r['failures'] == 0 and r['unchecked'] == 0 and r['worst'] <= 0.5, (c['id'], r)


@pytest.mark.parametrize('wrong', mc.ROOT_WRONG_FORMS)
@pytest.mark.parametrize('case_id', ['H-rays65-depth4-skip8', 'H-rays129-depth3-skip7', 'H-rays33-depth1-oct0'])
def test_wrong_root_finders_fail_the_trace_check(wrong, case_id):
    """The wrong bracket end moved, tau added, sigmoid(+10 x), the bracket's f rows swapped, one iteration too few."""
    c = [c for c in mc.H_CASES if c['id'] == case_id][0]
    net, inp = mc.root_inputs(c)
    r = mc.trace_check(net, inp, mc.root_find_definition(net, inp, mc.H_TRACE, wrong=wrong))
    assert not r['first_equal'] or r['failures'] > 0, (case_id, wrong, r)
    if wrong != 'swap_rows':
        assert r['first_equal'] and r['failures'] >= 5      # (the first estimate does not depend on these forms)
