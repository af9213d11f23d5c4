"""tests/lowp_cases.py without a GPU: the references satisfy the exactness conditions the bit-exact GPU tests rest on, the case
tables cover the edges of every launch path, and every exact case is sensitive -- a deliberately wrong model of the kernel
(two permuted K slots swapped, the low bias piece dropped, truncation instead of RNE, the lo plane dropped, group g reading group
0's bias, the ragged row tile reading row 0) changes at least one of its outputs."""
import numpy as np
import pytest
import torch

from tests import lowp_cases as lc


# --------------------------------------------------------------------------- exactness of the references
@pytest.mark.parametrize('c', lc.A_CASES, ids=lc.case_id)
def test_bf16_reference_is_exact(c):
    """reference_bf16 asserts, layer by layer: weights and tables are bf16 values, every bias is two bf16 pieces, every
    pre-activation is exact in fp32 in any order of accumulation and |z| <= 256, every integer-network activation equals its own
    bf16 round trip, the outputs are float32 values."""
    net, ref = lc.reference_bf16(c)
    assert ref['logit'].shape == (c['n'], net.n_out)
    if c['kind'] == 'int':
        acts = torch.cat([a.reshape(-1) for a in ref['acts']])
        assert float(acts.max()) <= 256 and 0.3 < float((acts != 0).double().mean()) < 0.9
        if c['n'] >= 31:
            assert ref['logit'].unique().numel() >= 8, 'the outputs are not diverse'


def test_probe_expectations_are_the_derived_ones():
    """The probe activations are DERIVED (lowp_cases.PROBES states them by hand); the reference reproduces them in every probe
    case, in the layer the probes sit in and -- carried by identity rows -- in the last hidden layer."""
    for c in lc.A2_CASES:
        net, ref = lc.reference_bf16(c)
        for o in range(31):
            want = lc.PROBES[o % 8][3]
            f = lc.probe_feature(o)
            assert bool((ref['acts'][c['lp']][:, f] == want).all()) and bool((ref['acts'][-1][:, f] == want).all()), (c['id'], o)
            assert bool((ref['logit'][:, o] == want + 0.5).all())
        g = torch.arange(c['n']) // c['maps'][2] % c['maps'][3]
        assert torch.equal(ref['logit'][:, 31], g.double() + 1.5)       # the group-dependent feature
    # round-half-up and truncation each give another value for one of the two ties
    up = lambda x: float(lc.bf16_trunc(torch.tensor(x + 2.0 ** -8)))     # round half up at this binade
    assert up(1.0 + lc.P8) != lc.PROBES[0][3] and float(lc.bf16_trunc(torch.tensor(1.0 + 3 * lc.P8))) != lc.PROBES[1][3]


@pytest.mark.parametrize('c', lc.B1_CASES, ids=lc.case_id)
def test_x3_reference_is_exact_and_pieces_do_not_overlap(c):
    """x3_reference asserts the selection structure and that every pre-activation is a float32; here the premise of the derived
    bit equality: for the case inputs (tables, the products U and w x_g made of them, biases -- whose three pieces meet inside ONE
    MFMA, and which the outputs of the wide cases read: test_every_hidden_bias_of_the_split_engine_is_observed --, weights) the
    three pieces add up to the operand in float32 in EVERY order.  The activations are sums U[n] + V[g] with
    arbitrary mantissas; their pieces arrive one per MFMA in the kernel's fixed order lo, mid, hi, which is exact for every
    float32: lo + mid is the residual x - hi, and the residual plus hi is x."""
    net, ref = lc.reference_x3(c)
    for t in [net.tab_a, net.tab_b] + ref['U'] + [b for b in net.bs] + [w for w in net.Ws]:
        assert lc.pieces_sum_exactly(t.contiguous())
    for a in ref['acts']:
        assert torch.equal(a.float().double(), a)
        hi, mid, lo = lc.split3(a.float())
        assert torch.equal((lo + mid) + hi, a.float()) and torch.equal(lo + mid, a.float() - hi)
    # full mantissas really travel: most outputs need more than 16 significant bits
    out = ref['out'].float()
    assert float((lc.r16(out) != out).double().mean()) > 0.3 or c['n'] * net.n_out < 8
    assert float((ref['acts'][-1] != 0).double().mean()) > 0.2


def test_order_free_condition_catches_inexact_sums():
    x = torch.tensor([[1.0, 2.0 ** -24]])
    w = torch.tensor([[1.0, 1.0]])
    with pytest.raises(AssertionError):
        lc.order_free([(x, w)])
    assert float(lc.order_free([(torch.tensor([[3.0, 2.0 ** -20]]), w)])) == 3.0 + 2.0 ** -20
    assert lc.lowbit(torch.tensor([6.0, 0.0, 1.25])) == 0.25


# --------------------------------------------------------------------------- coverage of the tables
def test_family_a_covers_the_listed_edges():
    twos = [c for c in lc.A1_TWO]
    assert {c['n'] for c in twos} >= set(lc.A_ROWS) == {1, 31, 32, 33, 64, 65, 255, 256, 257, 513}
    assert max(c['n'] for c in lc.A_CASES if c['form'] == 'two') <= 513
    assert {c['din'] for c in twos} >= {(63, 63), (64, 64), (1, 1), (33, 17), (40, 0)}
    assert {c['n_out'] for c in twos} >= {1, 2, 31, 32}
    maps = [c['maps'] for c in twos]
    assert any(m[0] == 1 and m[2] == m[1] and m[3] > 1 for m in maps)                        # a_div = 1, b_div = a_mod
    assert any(m[0] == 5 and m[0] * m[1] < lc.BF_TILE for m in maps)                         # a_div = 5, the wrap inside a tile
    assert any(m[3] == 1 and c['din'][1] > 0 for m, c in zip(maps, twos))                    # b_mod = 1
    assert any(c['din'][1] == 0 and lc.build_bf16(c).tab_b is None for c in twos)            # tab_b = None
    ds = {(c['depth'], c['skip_at']) for c in twos}
    assert any(d == 2 for d, _ in ds) and any(s == 0 for _, s in ds) and any(s == d - 3 and d > 3 for d, s in ds)
    assert any(s == lc.NO_SKIP and d > 2 for d, s in ds) and any(d == lc.MAX_HIDDEN + 1 for d, _ in ds)
    assert {c['out_act'] for c in lc.A_CASES if c['form'] == 'two'} == {'none', 'sigmoid', 'occ'} == {c['out_act'] for c in lc.A1_GROUPED}
    gr = {(c['rpg'], c['groups']) for c in lc.A1_GROUPED}
    assert gr >= {(r, g) for r in (1, 255, 256, 257) for g in (1, 3)}
    for c in lc.A1_GROUPED:   # the skip layer is present: two bias k-steps per group; table B differs per group
        assert 0 <= c['skip_at'] <= c['depth'] - 3
        net = lc.build_bf16(c)
        assert c['groups'] == 1 or len({tuple(r.tolist()) for r in net.tab_b}) == c['groups']
    assert {(c['form'], c['lp']) for c in lc.A2_CASES} == {(f, l) for f in ('two', 'grouped') for l in (0, 2, lc.PROBE_HIDDEN - 1)}
    for c in lc.A2_CASES:
        if c['form'] == 'grouped':     # the probe value arrives through the group table
            assert c['lp'] == 0 or c['skip_at'] == c['lp'] - 1
        else:                          # ... through the stream bias k-step of a layer that does not read the input block
            assert c['lp'] == 0 or c['skip_at'] != c['lp'] - 1


def test_input_block_edges_are_read():
    """The first and the last real column of each table's block are read by some weight of every input layer, and the columns
    behind them (zero-extended by the packer) hold non-zero table entries that a correct engine must ignore."""
    for c in lc.A1_TWO + lc.A1_GROUPED:
        net = lc.build_bf16(c)
        da, db = c['din']
        for li, W in enumerate(net.Ws[:-1]):
            if not lc._has_in(li, c['skip_at']):
                continue
            o = W.shape[1] - da - db
            cols = [o, o + da - 1] + ([o + da, o + da + db - 1] if db else [])
            assert all(bool((W[:, k] != 0).any()) for k in cols), (c['id'], li)
        if da < 64:
            assert bool((net.tab_a[:, da:] != 0).any())
        if db and db < 64 and c['form'] == 'two':
            assert bool((net.tab_b[:, db:] != 0).any())


def test_family_b_covers_the_listed_edges():
    assert {(c['rpg'], c['groups']) for c in lc.B1_CASES} >= {(r, g) for r in (1, 31, 32, 33, 127, 128, 129) for g in (1, 3)}
    assert max(c['rpg'] for c in lc.B1_CASES) <= 129
    ds = {(c['depth'], c['skip_at']) for c in lc.B1_CASES}
    for d in (3, 5, 12, lc.MAX_HIDDEN + 1):
        assert (d, 0) in ds and (d, lc.NO_SKIP) in ds
    assert any(0 < s < d - 3 for d, s in ds)                  # a skip in the middle
    assert {c['n_out'] for c in lc.B1_CASES} == {1, 3, 32}
    for it in lc.PACK_ITEMS:
        assert it['n_ot'] in (1, 8) and it['ks0'] + it['n_ks'] <= 16
    part = [it for it in lc.PACK_ITEMS if it['rows'] < 32 * it['n_ot'] and it['cols'] < 16 * (it['ks0'] + it['n_ks'])]
    assert {(it['permuted'], it['n_ot']) for it in part} == {(p, o) for p in (False, True) for o in (1, 8)}
    assert any(it['ks0'] > 0 for it in part if it['permuted']) and any(it['ks0'] > 0 for it in part if not it['permuted'])


# --------------------------------------------------------------------------- the layout models
def test_layout_model_is_a_permutation_of_the_source():
    """16 k-steps of either order visit every K index of a 256-column block exactly once per output row; the permuted order is the
    register layout of the header comment (feature 32 ot + 16 qp + 8 (j / 4) + 4 h + (j % 4) <-> k-step 2 ot + qp, slot 8 h + j)."""
    W = np.arange(256 * 256, dtype=np.float32).reshape(256, 256)
    for permuted in (False, True):
        src = lc.pack_source(W, permuted, 8, 0, 16)               # [ks, ot, lane, j]
        for ot in (0, 5):
            row = src[:, ot, :, :][:, [3, 35], :]                 # lanes 3 and 35: row 32 ot + 3, both lane halves
            assert sorted(row.reshape(-1).tolist()) == [float((32 * ot + 3) * 256 + k) for k in range(256)]
    for ot in range(8):
        for qp in range(2):
            for h in range(2):
                for j in range(8):
                    assert lc.k_index(True, 2 * ot + qp, h, j) == 32 * ot + 16 * qp + 8 * (j // 4) + 4 * h + (j % 4)
    # zero extension
    it = lc.PACK_ITEMS[0]
    _, view = lc.pack_matrix(it)
    src = lc.pack_source(view.numpy(), it['permuted'], it['n_ot'], it['ks0'], it['n_ks'])
    assert int((src == 0).sum()) >= (256 - it['rows']) * 128 + it['rows'] * (128 - it['cols'])
    planes = lc.pack_x3_reference(view.numpy(), it['permuted'], it['n_ot'], it['ks0'], it['n_ks'])
    p = torch.from_numpy(planes.copy()).view(torch.bfloat16).float().view(it['n_ks'], it['n_ot'], 3, 64, 8)
    assert torch.equal((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2], torch.from_numpy(src))
    V = lc.bias_matrix(3)
    for pieces in (2, 3):
        b = torch.from_numpy(lc.bias_step_reference(V, pieces).copy()).view(torch.bfloat16).float().view(3, 8, 64, 8)
        assert not bool(b[:, :, 32:, :].any()) and not bool(b[:, :, :, pieces:].any())
        hi = V.to(torch.bfloat16).float().view(3, 8, 32)
        assert torch.equal(b[:, :, :32, 0], hi) and torch.equal(b[:, :, :32, 1], (V.view(3, 8, 32) - hi).to(torch.bfloat16).float())
    assert torch.equal(b[..., 0] + b[..., 1] + b[..., 2], torch.nn.functional.pad(V.view(3, 8, 32), (0, 32)))


# --------------------------------------------------------------------------- sensitivity
def _changes(c, wrong):
    net, ref = lc.reference_bf16(c)
    return not torch.equal(lc.bf16_reference(net, wrong=wrong)['logit'], ref['logit'])


def test_swapped_k_slots_change_every_exact_case():
    for c in lc.A1_TWO + lc.A1_GROUPED:
        assert _changes(c, 'swap_k') or c['n'] == 1, c['id']
    W = lc.pack_matrix(lc.PACK_ITEMS[3])[1].numpy()
    it = lc.PACK_ITEMS[3]
    assert not np.array_equal(lc.pack_source(W, True, it['n_ot'], it['ks0'], it['n_ks'], swap=(133, 134)),
                              lc.pack_source(W, True, it['n_ot'], it['ks0'], it['n_ks']))


def test_dropped_bias_low_piece_changes_the_probe_cases():
    for c in lc.A2_CASES:
        assert _changes(c, 'no_bias_lo'), c['id']
    assert not _changes(lc.A1_TWO[3], 'no_bias_lo')     # (integer biases have no low piece: the probes are what sees it)


def test_truncation_changes_the_probe_cases():
    for c in lc.A2_CASES:
        assert _changes(c, 'trunc'), c['id']


def test_group_zero_bias_changes_every_grouped_case_with_more_groups():
    for c in lc.A1_GROUPED + [c for c in lc.A2_CASES if c['form'] == 'grouped']:
        assert _changes(c, 'group0_bias') == (c['groups'] > 1), c['id']


def test_ragged_tile_reading_row_zero_changes_the_ragged_cases():
    seen = 0
    for c in lc.A1_TWO + lc.A1_GROUPED:
        size = c['rpg'] if c['form'] == 'grouped' else c['n']
        ragged = size % lc.BF_TILE != 0 and size > 1
        assert _changes(c, 'clamp_row0') == ragged, c['id']
        seen += ragged
    assert seen >= 20


def _x3_changes(net, ref, **kw):
    return not torch.equal(lc.x3_reference(net, **kw)['out'], ref['out'])


def test_every_hidden_bias_of_the_split_engine_is_observed():
    """Multiplying ONE hidden layer's bias by 1.5 changes an output: for every hidden layer of every 32-output case (these cover
    every depth and skip position, the deepest network included), and for layer 1 and the last input layer's per-group bias in
    the 3-output cases.  The traced outputs differ from group to group where they carry a per-group bias."""
    wide = [c for c in lc.B1_CASES if c['n_out'] == 32]
    assert {(c['depth'], c['skip_at']) for c in wide} >= {(d, s) for d in (3, 5, 12, 13) for s in (0, lc.NO_SKIP)}
    for c in lc.B1_CASES:
        net, ref = lc.reference_x3(c)
        nh = c['depth'] - 1
        seen = [l for l in range(nh) if _x3_changes(net, ref, bias_scale=(l, 1.5))]
        if c['n_out'] == 32:
            assert seen == list(range(nh)), c['id']
            assert [(k, l) for _, k, l in net.traced if k == 'const'] == [('const', l) for l in range(nh)]
        elif c['n_out'] == 3:
            last_in = max(l for l in range(nh) if lc._has_in(l, c['skip_at']))
            assert 1 in seen and last_in in seen, c['id']
        for o, kind, l in net.traced:
            col = ref['out'][:, o].reshape(c['groups'], c['rpg'])
            assert bool((col == col[:, :1]).all())                                   # a bias: the same for every row of a group
            if kind == 'group' and c['groups'] > 1:
                assert col[:, 0].unique().numel() == c['groups'], c['id']            # ... and another one for every group


def test_wrong_bias_models_change_the_split_cases():
    """The stream bias k-step without its lo piece, the previous layer's bias k-step, group 0's V row for every group, the first
    input layer's tables for the second: each changes an output of every case that reads the biases and has such a path."""
    n = dict.fromkeys(lc.WRONG_X3, 0)
    for c in lc.B1_CASES:
        if c['n_out'] != 32:
            continue
        net, ref = lc.reference_x3(c)
        stream = any(not lc._has_in(l, c['skip_at']) for l in range(c['depth'] - 1))
        expect = dict(bias_no_lo=stream, bias_wrong_layer=stream, group0=c['groups'] > 1, in_idx0=0 <= c['skip_at'] < c['depth'] - 2)
        for k, e in expect.items():
            assert _x3_changes(net, ref, wrong=k) == e, (c['id'], k)
            n[k] += e
    assert min(n[k] for k in ('bias_no_lo', 'bias_wrong_layer', 'group0', 'in_idx0')) >= 4


def test_occupancy_bias_networks_observe_their_layer():
    """B2-bias-layer l: the output is the bias of hidden layer l handed on -- scaling that bias changes it, in float64."""
    from tests import mlp_cases as mc
    assert [c['trace'] for c in lc.B2_BIAS_CASES] == [0, 1, 2, 3] and all(c['depth'] == 5 and c['skip'] == 2 for c in lc.B2_BIAS_CASES)
    for c in lc.B2_BIAS_CASES:
        net = lc.build_occ_net(c)
        ev = lambda bs: mc.evaluate(mc.net_from_geo(net.Ws, bs, net.skips, lc.OCC_OCTAVES, net.points, lc.OCC_SCALE), torch.float64)['out']
        base = ev(net.bs)
        assert 0.02 < float(base.min()) and float(base.max()) < 0.98
        for l in range(4):
            bs = [b * 1.5 if i == l else b for i, b in enumerate(net.bs)]
            assert (not torch.equal(ev(bs), base)) == (l == c['trace']), (c['id'], l)


def test_dropped_lo_plane_changes_every_split_case():
    for c in lc.B1_CASES:
        net, ref = lc.reference_x3(c)
        assert not torch.equal(lc.x3_reference(net, wrong='no_lo')['out'], ref['out']), c['id']


# --------------------------------------------------------------------------- B2 and C
def test_occupancy_networks_are_selection_networks():
    part = lc.sqrt2_partner()
    inv = 1.0 / 2.0 ** 0.5
    assert float((torch.tensor([part]) * inv)[0]) == 1.0 and abs(part - 2.0 ** 0.5) < 1e-6
    assert tuple(c['n'] for c in lc.B2_POINT_CASES[:8]) == lc.OCC_ROWS == (0, 1, 31, 32, 33, 127, 128, 129)
    assert min(lc.OCC_COUNTS) < lc.OCC_CAPACITY < max(lc.OCC_COUNTS) and lc.OCC_CAPACITY in lc.OCC_COUNTS
    for c in lc.B2_POINT_CASES + lc.B2_BIAS_CASES + [lc.occ('B2-indirect', n=lc.OCC_CAPACITY), lc.occ('B2-sweep', sweep=True)]:
        net = lc.build_occ_net(c)
        sk = c['skip']
        assert net.Ws[sk - 1].shape[0] == lc.OCC_PE_FIRST and net.Ws[sk].shape[1] == 256 and net.Ws[0].shape[1] == lc.OCC_DPE
        for li, (W, b) in enumerate(zip(net.Ws, net.bs)):
            Wf = W * inv if li == sk else W
            assert int((W != 0).sum(1).max()) == 1
            assert torch.equal(lc.bf16(Wf), Wf) and bool((torch.frexp(Wf[Wf != 0])[0].abs() == 0.5).all())      # +-2^e after the fold
            if li < len(net.Ws) - 1:
                assert not bool(((W != 0).any(1) & (b != 0)).any())
            assert lc.pieces_sum_exactly(b)
        assert int((net.Ws[-1] != 0).sum()) == 1


def test_sweep_rays_are_the_four_kinds():
    """In float64: kind 0 changes sign across the 128-step block boundary (256 steps; no workgroup sees it), kind 1 starts
    occupied, kind 2 never crosses, kind 3 crosses inside the first block."""
    from tests import mlp_cases as mc
    assert lc.SWEEP_STEPS == (128, 256) and lc.SWEEP_RAYS == (1, 3, 70)
    net = lc.build_occ_net(lc.occ('B2-sweep', sweep=True))
    for M in lc.SWEEP_STEPS:
        s = lc.sweep_rays(70, M)
        pts = mc.sweep_points(s['origin'], s['direction'], s['far'], s['u'], s['omu'], torch.tensor(s['near']))
        o = mc.evaluate(mc.net_from_geo(net.Ws, net.bs, net.skips, lc.OCC_OCTAVES, pts, lc.OCC_SCALE), torch.float64)['out'].reshape(70, M)
        idx, blk = lc.first_change(o - 0.5)
        k = s['kind']
        assert bool((idx[k == 1] == 0).all()) and bool((blk[k == 1] == 0).all())
        assert bool((idx[k == 2] == -1).all()) and bool((blk[k == 2] == -1).all())
        assert bool(((idx[k == 3] > 0) & (idx[k == 3] < 127)).all()) and bool((blk[k == 3] == 0).all()) and idx[k == 3].unique().numel() > 4
        if M == 256:
            assert bool((idx[k == 0] == 127).all()) and bool((blk[k == 0] == -1).all())
        else:
            assert bool((idx[k == 0] == 126).all()) and bool((blk[k == 0] == 0).all())
        # the margin: no occupancy closer to 1/2 than 1e-3, so float32 evaluations see the same signs
        assert float((o - 0.5).abs().min()) > 1e-3


def test_family_c_model_and_cases():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 64, generator=g) * 3
    w = torch.randn(5, 64, generator=g)
    assert torch.equal(lc.r16(lc.r16(x)), lc.r16(x)) and not torch.equal(lc.r16(x), x)
    xh, wh = lc.bf16(x), lc.bf16(w)
    xm, wm = lc.bf16(x - xh), lc.bf16(w - wh)
    d = lambda a, b: a.double() @ b.double().t()
    want = d(xh, wh) + d(xh, wm) + d(xm, wh)
    assert torch.equal(lc.x3dot(x, w, torch.float64), want)
    full = d(x, w)
    e3, e1 = float((want - full).abs().max()), float((d(xh, wh) - full).abs().max())
    l1 = float(d(x.abs(), w.abs()).max())
    # dropped: hi lo-ish terms of 2^-16 |x w| each and smaller (three products); a bf16 operand rounding of 2^-9 each (one product)
    assert e3 <= 2.0 ** -15 * l1 and e1 > 20 * e3
    # a weight without a mid piece: the model is the exact product with r16(x)
    w2 = torch.where(torch.rand(5, 64, generator=g) < 0.5, 2.0, -0.5)
    assert torch.equal(lc.x3dot(x, w2, torch.float64), d(lc.r16(x), w2))
    assert {c['n'] for c in lc.C1_CASES if c['form'] == 'lean' and not c['precompute']} == {1, 63, 64, 65, 129}
    assert max(c['n'] for c in lc.C1_CASES) <= 129
    assert {c['form'] for c in lc.C1_CASES} == {'lean', 'padded', 'orders'} and any(c['precompute'] and c['form'] == 'lean' for c in lc.C1_CASES)
    pad = [c for c in lc.C1_CASES if c['form'] == 'padded'][0]
    assert 0 < pad['live'] % 64 and pad['live'] < pad['period'] - 64       # a live count in the middle of a period: one block is all padding
    for c in lc.C1_CASES:
        net = lc.build_x3_net(c)
        for W in net.Ws:
            assert int((W != 0).sum(1).max()) == 1, c['id']     # one weight per row over [activations | table A | table B]
        lc.x3_reference(net)


def test_family_c_reference_arithmetic_holds_half_the_bound():
    """The float32 evaluation of the modelled arithmetic stays within half of rtol 1e-5 x max of the float64 one in every tensor of
    the C2 chain: the kernel is then allowed no element beyond the bound (helpers.assert_vs_truth)."""
    from tests import mlp_cases as mc
    from tests.helpers import truth_ratios
    Ws, bs = lc.geo_weights(7)
    pts = torch.rand(129, 3, generator=torch.Generator().manual_seed(3)) * 2 - 1
    xs32 = pts * torch.tensor(lc.OCC_SCALE, dtype=torch.float32)
    pe = mc.pe_columns(xs32, lc.OCC_OCTAVES, torch.float32)
    t64, t32 = lc.geo_chain_model(Ws, bs, 2, pe, torch.float64), lc.geo_chain_model(Ws, bs, 2, pe, torch.float32)
    for a, b in [(t64[0], t32[0]), (t64[1], t32[1])] + list(zip(t64[2], t32[2])):
        _, r_ref, _, _, _ = truth_ratios(b.numpy(), b.numpy(), a.numpy(), mc.RTOL, 'max')
        assert float(r_ref.max()) < 0.5, float(r_ref.max())
