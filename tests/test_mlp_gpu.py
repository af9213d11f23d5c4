"""The fused MLP engine (csrc/mlp_infer.hip) against float64, launch path by launch path, on the cases of tests/mlp_cases.py
(whose coverage of the dispatcher tests/test_mlp_cpu.py asserts without a GPU): the packers bit for bit against the stage order of
the header comment, the lean engine (plain, index maps, dumps and sign bits, padded row sets, both block orders), the chain-only
features (rank-k init, dump tile masks, the 33..64-output final layer, the single-dump programs, masks as tensors and as sign
bits, initial activations), the encoding prologue (psn_mlp_infer_pe, its indirect form, psn_march_sweep), the secant root finder
(psn_root_find) in both forms and the argument checks.

The root finder (family H: eleven small networks, 1 .. 129 rays, 1 .. 11 hidden layers, layers of 10, 9, 8 and 7 weight stages, brackets
found on the CPU by sweeping the float64 definition, a few benign and degenerate brackets in every case).  D[k] = the depths after k
iterations.  (a) root_find_fp_kernel (16 rays per workgroup, the default) and mlp_infer_kernel<false, 16, 1> (64 rays per workgroup,
under PSN_ROOT_FIND_ROW_PARALLEL=1) write the same bits at k = 0, 1, 2, 3, 8, 64; (b) nothing but the n depths is written; (c) D[0] ..
D[8] of both forms equal the composition psn_secant_step / psn_mlp_infer_pe / psn_secant_step BIT FOR BIT -- measured on the first
run on an MI355X: no iterate of any case differs, so equality is asserted, and the 1e-6 of
test_stage1_gpu.test_root_finder_and_crossing_vs_stepwise_formulation became torch.equal; (d) D[0] .. D[3] of the crossing rays pass
mlp_cases.trace_check, the teacher-forced float64 check (its docstring has the rule): the figures of the two src1 / src4 rows below are
the worst |D[k + 1] - d'| / a' and the float32 CPU definition's worst in the same case.  From iterate 4 on stuck iterates divide by
zero in the float64 candidates, which is why (d) stops at 3 and (c) carries the rest.  A division by zero in the bracket (f_low ==
f_high) gives inf and, from the first occupancy on, NaN -- except in a ReLU network, where v_max_f32 answers max(NaN, 0) = 0 and the
depth stays inf; the forms agree on which.

Bound: helpers.assert_vs_truth, rtol 1e-5, atol 'max', per tensor, with the float32 CPU definition as the reference arithmetic;
test_mlp_cpu.py shows that this reference never passes half the bound, so the kernel is allowed no element beyond it.  Every
output and dump buffer starts as NaNs of a fixed bit pattern inside a larger buffer: what the launch must not write keeps its bits.

Measured worst r_hip per instantiation (units of the bound) on an MI355X:
    instantiation          r_hip   r_ref   worst tensor
    chain/16               0.140   0.045   F-wide33 second1
    chain/16/froma         0.065   0.017   F-mul2_a dump1
    chain/16/trim          0.060   0.024   F-chain-trim second1
    chain/16/trim/froma    0.041   0.028   F-froma-trim out
    chain/4                0.017   0.022   F-act_init-w64 dump1
    chain/8                0.082   0.045   F-tiles-w128-ffff second1
    lean/16                0.088   0.057   C-pair-P128-G3-init out
    lean/16/src2/trim      0.104   0.038   G-rows129 out
    lean/16/src3/trim      0.117   0.058   G-sweep-rays3-steps192 occ
    lean/16/src1/trim      0.199   0.109   H-rays17-depth4-trim ray 13 D[2]   (units of the allowance a' of trace_check)
    lean/16/src4/trim      0.199   0.109   H-rays17-depth4-trim ray 13 D[2]   (the same bits as src1, as (a) asserts)
    lean/16/trim           0.076   0.037   B-trim217 out
    lean/4                 0.134   0.021   B-rows1-w64 out
    lean/8                 0.711   0.133   B-rows1-w128 out   (one row, one output: the bound is purely relative there)
254 tests, 4.3 s of wall time for the module (the 42 root-finder tests: 1.2 s).

Family H found no defect in either form of the root finder.  One change of the library came with it: psn_root_find on no rays
now clears the thread's last path, so that psn_mlp_last_path does not answer with an earlier launch.

Finding of this suite (fixed in csrc/mlp_infer.hip, cases C-pointmajor-rows and C-pointmajor-rows-G7 kept): the lean engine took the
B-side init row through LDS whenever the first and the last row of a workgroup mapped to the same B-table row.  With b_div * b_mod
< 64 (point-major rows, b_div = 1) the index wraps inside the block -- 63 % 3 == 63 % 7 == 0 -- and all 64 rows were given the
init row of the first one (168 of 300 outputs wrong, up to 6e4 x the bound).  The test is now the same quotient row / b_div.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from tests import mlp_cases as mc
from tests.helpers import assert_vs_truth

pytestmark = pytest.mark.gpu
_WORST = {}      # instantiation -> (worst r_hip, r_ref there, case and tensor)
NAN_BITS = 0x7FC12345
G_OUT, G_DUMP = mc.GUARD, 130   # guard rows (dumps: more than the largest save_row0, a row index taken without it lands there)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _WORST:
        print('\n==== fused MLP engine vs float64: worst r_hip per instantiation (r_ref in the same tensor), in units of the bound ====')
        for name, (rh, rr, where) in sorted(_WORST.items()):
            print('%-22s r_hip %6.3f  r_ref %6.3f  (%s)' % (name, rh, rr, where))


@pytest.fixture(scope='module')
def mods(cuda):
    from psnerf_amd import hip, fused
    return hip, fused


def nan_buffer(rows, cols, cuda, guard):
    """(whole, view): ``rows`` x ``cols`` floats of NAN_BITS with ``guard`` rows of the same in front and behind."""
    whole = torch.full((rows + 2 * guard, cols), NAN_BITS, dtype=torch.int32, device=cuda).view(torch.float32)
    return whole, whole[guard:guard + rows]


def untouched(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


def guards_intact(whole, rows, guard):
    return untouched(whole[:guard]) and untouched(whole[guard + rows:])


def check(c, path, name, got, truth, ref):
    got = got.detach().cpu().numpy()
    assert got.shape == tuple(truth.shape), '%s %s: shape %s vs %s' % (c['id'], name, got.shape, tuple(truth.shape))
    rh, rr = assert_vs_truth('%s %s' % (c['id'], name), got, ref.numpy(), truth.numpy(), mc.RTOL, 'max')
    print('%s %-10s r_hip %.3f r_ref %.3f' % (c['id'], name, rh, rr))
    if rh > _WORST.get(path, (-1.0,))[0]:
        _WORST[path] = (rh, rr, '%s %s' % (c['id'], name))


def assert_path(c, net, path, **kw):
    """What the library launched (PsnMlpPath) is the instantiation mlp_cases.dispatch states for the case."""
    d = mc.dispatch(c, net, **kw)
    assert path.blocks > 0, '%s: nothing was launched' % c['id']
    assert 'blocks' not in d or path.blocks == d['blocks'], '%s: a grid of %d workgroups' % (c['id'], path.blocks)
    got = dict(chain=bool(path.chain), hid=path.width16 // 2, src=path.src, trim=bool(path.trim), from_a=bool(path.from_a),
               point_major=path.pm_period != 0)
    assert got == {k: d[k] for k in got}, '%s: launched %s' % (c['id'], got)
    name = '%s/%d%s%s%s' % ('chain' if path.chain else 'lean', path.width16, '/src%d' % path.src if path.src else '',
                            '/trim' if path.trim else '', '/froma' if path.from_a else '')
    assert name == d['name'], c['id']


def pack_net(net, mods, cuda):
    hip, fused = mods
    names = dict(none='NONE', relu='RELU', softplus='SOFTPLUS100')
    code = lambda a: getattr(hip, 'ACT_' + names.get(a, a.upper()))
    spec = net.pack_spec(lambda t: t.to(cuda), code, fused.DIRECT_INIT)
    pk = fused.pack_layers(spec, net.ka, net.kb, net.n_out, getattr(hip, 'OUT_' + net.out_act.upper()), cuda,
                           has_final=net.n_out > 0, width=net.width)
    for l, L in enumerate(net.layers):
        assert pk.desc.layers[l].act == mc.ACT[L['act']]
    assert [(pk.desc.layers[l].n_kt_in, pk.desc.layers[l].n_kt_act, pk.desc.layers[l].init_off >= 0)
            for l in range(len(net.layers))] == mc.layer_shape(net)
    return pk


# --------------------------------------------------------------------------- A: the packers
def _pack_views(items, cuda):
    views = []
    for it in items:
        store, view = mc.pack_matrix(it)
        v = store.to(cuda)[:, it['col0']:it['col0'] + view.shape[1]]
        assert v.stride(0) == view.shape[1] + it['ldw_extra'] and v.stride(1) == 1
        views.append((v, mc.pack_reference(view.numpy(), it['n_mt'], it['k_tiles'], it['transpose'])))
    return views


def _same_bits(got, ref):
    return np.array_equal(got.cpu().numpy().view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize('item', mc.PACK_ITEMS, ids=mc.case_id)
def test_pack_layer_equals_stage_order(mods, cuda, item):
    hip, _ = mods
    (v, ref), = _pack_views([item], cuda)
    size = item['n_mt'] * item['k_tiles'] * 1024
    whole, dst = nan_buffer(1, size, cuda, 1)
    hip.mlp_pack_layer(v, item['n_mt'], item['k_tiles'], dst[0], transpose=item['transpose'])
    assert _same_bits(dst[0], ref) and guards_intact(whole, 1, 1)
    # the grouped packer on the same block, alone
    whole2, dst2 = nan_buffer(1, size, cuda, 1)
    hip.mlp_pack_layers([(v, item['transpose'], item['n_mt'], item['k_tiles'], dst2[0])])
    assert _same_bits(dst2[0], ref) and guards_intact(whole2, 1, 1)


@pytest.mark.parametrize('n_items', mc.PACK_GROUP_SIZES)
def test_pack_layers_groups(mods, cuda, n_items):
    """1, 24 (one full launch) and 25 items (a second launch): every block equals the single packer's reference, the floats
    between the blocks keep their bits."""
    hip, _ = mods
    items = [mc.PACK_ITEMS[i % len(mc.PACK_ITEMS)] for i in range(n_items)]
    views = _pack_views(items, cuda)
    gap = 4
    sizes = [it['n_mt'] * it['k_tiles'] * 1024 for it in items]
    whole = torch.full((sum(sizes) + gap * (n_items + 1),), NAN_BITS, dtype=torch.int32, device=cuda).view(torch.float32)
    plan, offs, o = [], [], gap
    for it, (v, _), sz in zip(items, views, sizes):
        plan.append((v, it['transpose'], it['n_mt'], it['k_tiles'], whole[o:o + sz]))
        offs.append(o)
        o += sz + gap
    hip.mlp_pack_layers(plan)
    for it, (_, ref), sz, o in zip(items, views, sizes, offs):
        assert _same_bits(whole[o:o + sz], ref), it['id']
        assert untouched(whole[o - gap:o]) and untouched(whole[o + sz:o + sz + gap]), it['id']


# --------------------------------------------------------------------------- B - E: the lean engine
def run_lean(c, net, pk, mods, cuda, order=None, live=None, dumps=True, res=None):
    hip, _ = mods
    n = c['n']
    a_div, a_mod, b_div, b_mod = net.maps
    ta = net.tab_a.to(cuda)
    tb = None if net.tab_b is None else net.tab_b.to(cuda)
    res = {} if res is None else res   # (the caller's dict: the buffers stay inspectable when the launch is refused)
    res['bufs'] = []
    whole, out = nan_buffer(n, net.n_out, cuda, G_OUT)
    res['bufs'].append((whole, n, G_OUT))
    row0 = c['save_row0'] if c['save_row0'] is not None else 0
    save = bits = None
    if dumps and c['save'] is not None:
        save, bits = [], []
        want_bits = c['bits'] if isinstance(c['bits'], tuple) else (bool(c['bits']),) * len(c['save'])
        for l, on in enumerate(c['save']):
            if not on:
                save.append(None)
                bits.append(None)
                continue
            w_, d_ = nan_buffer(n - row0, net.width, cuda, G_DUMP)
            res['bufs'].append((w_, n - row0, G_DUMP))
            save.append(d_)
            bits.append(torch.full((n - row0, 4), -1, dtype=torch.int64, device=cuda) if want_bits[l] else None)
        if not any(b is not None for b in bits):
            bits = None
    kw = {}
    if live is not None:
        kw['live'] = (torch.tensor([float(live)], device=cuda), c['period'])
    path = hip.PsnMlpPath()
    call = lambda: pk(ta, n, a_div=a_div, a_mod=a_mod, tab_b=tb, b_div=b_div, b_mod=b_mod, out=out, save=save,
                      save_row0=row0, save_bits=bits, path=path, **kw)
    if order is None:
        call()
    else:
        with hip.block_order(order):
            call()
    assert_path(c, net, path, point_major=order != 'row', live=live)
    res.update(out=out, save=save, bits=bits)
    for w_, rows, g_ in res['bufs']:
        assert guards_intact(w_, rows, g_), '%s: a guard row was written' % c['id']
    return res


def equal_results(a, b):
    ok = torch.equal(a['out'].view(torch.int32), b['out'].view(torch.int32))
    for x, y in zip(a['save'] or [], b['save'] or []):
        ok = ok and (x is None or torch.equal(x.view(torch.int32), y.view(torch.int32)))
    for x, y in zip(a['bits'] or [], b['bits'] or []):
        ok = ok and (x is None or torch.equal(x, y))
    return ok


@pytest.mark.parametrize('c', mc.LEAN_CASES, ids=mc.case_id)
def test_lean_engine_vs_float64(mods, cuda, c):
    net, t64, t32 = mc.reference(c)
    pk = pack_net(net, mods, cuda)
    path = mc.dispatch(c, net)['name']
    first = None
    for order in c['orders']:
        r = run_lean(c, net, pk, mods, cuda, order=order)
        if first is not None:
            assert equal_results(r, first), '%s: block order %s changes the result' % (c['id'], order)
            continue
        first = r
        check(c, path, 'out', r['out'], t64['out'], t32['out'])
        row0 = c['save_row0'] or 0
        for l, d in enumerate(r['save'] or []):
            if d is None:
                continue
            check(c, path, 'dump%d' % l, d, t64['d1'][l][row0:], t32['d1'][l][row0:])
            if r['bits'] is not None and r['bits'][l] is not None:
                # the words of the header's formula, applied to the kernel's own dump
                assert np.array_equal(r['bits'][l].cpu().numpy(), mc.sign_words(d.cpu().numpy())), '%s: sign bits of layer %d' % (c['id'], l)
        if c['save'] is not None:
            # the rows ride along: the launch without dumps gives the same outputs bit for bit
            plain = run_lean(c, net, pk, mods, cuda, order=order, dumps=False)
            assert torch.equal(plain['out'].view(torch.int32), r['out'].view(torch.int32))


@pytest.mark.parametrize('c', mc.E_CASES, ids=mc.case_id)
def test_padded_row_sets(mods, cuda, c):
    """PsnMlpLaunch.live_count: the all-padding blocks (stated from live and period) are exact zeros, every other row and every dump
    equals the plain launch bit for bit, in both block orders; the plain launch meets the float64 bound."""
    net, t64, t32 = mc.reference(c)
    pk = pack_net(net, mods, cuda)
    path = mc.dispatch(c, net)['name']
    plain = run_lean(c, net, pk, mods, cuda, order='row')
    check(c, path, 'out', plain['out'], t64['out'], t32['out'])
    row0 = c['save_row0']
    for l, d in enumerate(plain['save'] or []):
        check(c, path, 'dump%d' % l, d, t64['d1'][l][row0:], t32['d1'][l][row0:])
    for order in c['orders']:
        assert equal_results(run_lean(c, net, pk, mods, cuda, order=order), plain)
        for live in c['live']:
            r = run_lean(c, net, pk, mods, cuda, order=order, live=live)
            dead = torch.from_numpy(mc.dead_rows(c, live)).to(cuda)
            what = '%s order=%s live=%d' % (c['id'], order, live)
            assert bool((r['out'][dead].view(torch.int32) == 0).all()), what + ': a dead block is not exact zeros'
            assert torch.equal(r['out'][~dead].view(torch.int32), plain['out'][~dead].view(torch.int32)), what + ': live rows differ'
            for x, y in zip(r['save'] or [], plain['save'] or []):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what + ': dumps differ'


# --------------------------------------------------------------------------- F: chain-only features
def run_chain(c, net, pk, mods, cuda, masks=None, res=None):
    hip, _ = mods
    n, W, nl = c['n'], net.width, len(net.layers)
    nh = net.n_hidden
    dv = lambda t: None if t is None else t.to(cuda)
    res = {} if res is None else res   # (the caller's dict: the buffers stay inspectable when the launch is refused)
    res['bufs'] = []
    out = None
    if net.n_out > 0:
        whole, out = nan_buffer(n, net.n_out, cuda, G_OUT)
        res['bufs'].append((whole, n, G_OUT))
    save, save2 = [], []
    for l in range(nl):
        L = net.layers[l]
        hidden = l < nh
        for lst, on in ((save, hidden), (save2, hidden and L['act'] in mc.SECOND)):
            if on:
                w_, d_ = nan_buffer(n, W, cuda, G_OUT)
                res['bufs'].append((w_, n, G_OUT))
                lst.append(d_)
            else:
                lst.append(None)
    save = save[:nh]
    mask = [dv(masks[l]) if (masks is not None and l in masks) else dv(net.mask.get(l)) for l in range(nl)]
    aux2 = [dv(net.aux2.get(l)) for l in range(nl)]
    kw = {}
    if c['tile_masks'] is not None:
        kw['save_tiles'], kw['save2_tiles'] = [c['tile_masks'][0]] * nh, [c['tile_masks'][1]] * nh
    elif c['force_chain']:
        kw['save_tiles'] = []
    if net.rk is not None:
        kw['rank_init'] = (dv(net.rk[0]).contiguous(), dv(net.rk[1]).contiguous())
    path = hip.PsnMlpPath()
    hip.mlp_infer(pk.desc, pk.w, pk.b, dv(net.tab_a), 1, n, None, 1, 1, n, out=out, init_a=dv(net.init_direct), save=save, save_row0=0,
                  mask=mask if any(m is not None for m in mask) else None, aux2=aux2 if any(m is not None for m in aux2) else None,
                  save2=save2 if any(m is not None for m in save2) else None, act_init=dv(net.act_init),
                  act_init_rows=net.act_init_rows, path=path, **kw)
    assert_path(c, net, path)
    for w_, rows, g_ in res['bufs']:
        assert guards_intact(w_, rows, g_), '%s: a guard row was written' % c['id']
    res.update(out=out, save=save, save2=save2)
    return res


def tile_columns(mask, W):
    cols = np.zeros(W, dtype=bool)
    for mt in range(W // 16):
        if (mask >> mt) & 1:
            cols[16 * mt:16 * mt + 16] = True
    return cols


@pytest.mark.parametrize('c', mc.F_CASES, ids=mc.case_id)
def test_chain_features_vs_float64(mods, cuda, c):
    net, t64, t32 = mc.reference(c)
    masks = None
    if c['bits_from_lean']:
        # the masks of a RELU_BITS chain: the sign-bit words a lean forward of the same width left behind; the definition reads
        # that launch's dumps
        src = mc.lean(c['id'] + '-forward', n=c['n'], width=c['width'], depth=2, skip=None, save_row0=0, save=(True, True), bits=True, n_out=1)
        snet = mc.build(src)
        fwd = run_lean(src, snet, pack_net(snet, mods, cuda), mods, cuda)
        net = mc.build(c)
        net.mask = {l: fwd['save'][l].cpu() for l in range(2)}
        masks = {l: fwd['bits'][l] for l in range(2)}
        t64, t32 = mc.evaluate(net, torch.float64), mc.evaluate(net, torch.float32)
    pk = pack_net(net, mods, cuda)
    path = mc.dispatch(c, net)['name']
    r = run_chain(c, net, pk, mods, cuda, masks=masks)
    W = net.width
    m1, m2 = c['tile_masks'] if c['tile_masks'] is not None else (0xFFFF, 0xFFFF)
    want = dict(mc.checked_tensors(c, t64))
    ref = dict(mc.checked_tensors(c, t32))
    if net.n_out > 0:
        check(c, path, 'out', r['out'], want['out'], ref['out'])
    for l in range(net.n_hidden):
        for key, buf, m in (('dump%d' % l, r['save'][l], m1), ('second%d' % l, r['save2'][l], m2)):
            if buf is None:
                continue
            sel = torch.from_numpy(tile_columns(m, W))
            dsel = sel.to(cuda)
            assert untouched(buf[:, ~dsel]), '%s %s: an unselected dump tile was written' % (c['id'], key)
            check(c, path, key, buf[:, dsel], want[key][:, sel], ref[key][:, sel])


# --------------------------------------------------------------------------- G: the encoding prologue
@pytest.mark.parametrize('c', mc.G_CASES, ids=mc.case_id)
def test_encoding_prologue_vs_float64(mods, cuda, c):
    hip, _ = mods
    net, t64, t32 = mc.reference(c)
    pk = pack_net(net, mods, cuda)
    path = mc.dispatch(c, net)['name']
    pts = net.points.to(cuda).contiguous()
    launched = hip.PsnMlpPath()
    if c['src'] == 3:
        s = net.sweep
        occ, skip = hip.march_sweep(pk.desc, pk.w, pk.b, s['origin'].to(cuda), s['direction'].to(cuda), s['far'].to(cuda), s['u'].to(cuda),
                                    s['omu'].to(cuda), s['near'], c['steps'], 0.5, c['octaves'], c['pe_scale'], early_exit=False, path=launched)
        assert_path(c, net, launched)
        assert skip is None and occ.shape == (c['rays'], c['steps'])
        check(c, path, 'occ', occ.reshape(-1, 1), t64['out'], t32['out'])
        # the same points through the table-free point launch: bit-identical
        direct = pk.on_points(pts, c['octaves'], c['pe_scale'])
        assert torch.equal(direct.view(torch.int32), occ.reshape(-1, 1).view(torch.int32))
        return
    Q = pts.shape[0]
    whole, out = nan_buffer(Q, net.n_out, cuda, G_OUT)
    pk.on_points(pts, c['octaves'], c['pe_scale'], out=out, path=launched)
    assert_path(c, net, launched)
    assert guards_intact(whole, Q, G_OUT)
    if c['count'] is None:
        check(c, path, 'out', out, t64['out'], t32['out'])
        return
    cnt = c['count']
    count = torch.tensor([cnt], dtype=torch.int64, device=cuda)
    if not c['scatter']:
        w2, o2 = nan_buffer(Q, net.n_out, cuda, G_OUT)
        pk.on_points(pts, c['octaves'], c['pe_scale'], out=o2, n_rows_dev=count, path=launched)
        assert guards_intact(w2, Q, G_OUT) and untouched(o2[cnt:]), '%s: a row behind the count was written' % c['id']
        got = o2[:cnt]
    else:
        perm = torch.randperm(mc.SCATTER_ROWS, generator=torch.Generator().manual_seed(cnt))[:Q].to(cuda)
        w2, o2 = nan_buffer(mc.SCATTER_ROWS, net.n_out, cuda, G_OUT)
        pk.on_points(pts, c['octaves'], c['pe_scale'], out=o2, n_rows_dev=count, out_rows=perm, path=launched)
        named =torch.zeros(mc.SCATTER_ROWS, dtype=torch.bool, device=cuda)
        named[perm[:cnt]] = True
        assert guards_intact(w2, mc.SCATTER_ROWS, G_OUT) and untouched(o2[~named]), '%s: an entry no out_rows names was written' % c['id']
        got = o2[perm[:cnt]]
    assert_path(c, net, launched)
    assert torch.equal(got.view(torch.int32), out[:cnt].view(torch.int32)), '%s: differs from the plain launch' % c['id']
    check(c, path, 'out', got, t64['out'][:cnt], t32['out'][:cnt])


# --------------------------------------------------------------------------- H: the secant root finder, both forms
ROOT_FORMS = (False, True)     # row_parallel: False = root_find_fp_kernel (the default), True = mlp_infer_kernel<false, 16, 1> (the hook)
_ROOT_D = {}                   # (case id, row_parallel, n_iter) -> D[n_iter] as float32 ndarray [n]
ROOT_TAIL = 70                 # rows behind the n outputs, inside the NaN buffer: more than a workgroup of either form


@contextlib.contextmanager
def root_form(row_parallel):
    """The library's hook PSN_ROOT_FIND_ROW_PARALLEL (read at every call) set to the wanted form around the calls."""
    old = os.environ.pop('PSN_ROOT_FIND_ROW_PARALLEL', None)
    if row_parallel:
        os.environ['PSN_ROOT_FIND_ROW_PARALLEL'] = '1'
    try:
        yield
    finally:
        os.environ.pop('PSN_ROOT_FIND_ROW_PARALLEL', None)
        if old is not None:
            os.environ['PSN_ROOT_FIND_ROW_PARALLEL'] = old


def root_device(c, mods, cuda):
    net, inp = mc.root_inputs(c)
    dev = {k: torch.from_numpy(inp[k]).to(cuda).contiguous() for k in ('origin', 'direction', 'bracket')}
    return net, inp, pack_net(net, mods, cuda), dev


def root_depths(c, net, inp, pk, dev, mods, cuda, n_iter, row_parallel):
    """D[n_iter] of one form: one launch into a NaN buffer.  (b): the guard rows and the ROOT_TAIL rows behind the n outputs keep their
    bits; the launch is the instantiation and the grid mlp_cases.dispatch states for the form."""
    key = (c['id'], row_parallel, n_iter)
    if key not in _ROOT_D:
        hip, _ = mods
        n = c['n']
        whole, view = nan_buffer(n + ROOT_TAIL, 1, cuda, G_OUT)
        path = hip.PsnMlpPath()
        with root_form(row_parallel):
            hip.root_find(pk.desc, pk.w, pk.b, dev['origin'], dev['direction'], dev['bracket'], inp['tau'], n_iter, c['octaves'],
                          c['pe_scale'], out=view[:n].reshape(-1), path=path)
        assert_path(c, net, path, row_parallel=row_parallel)
        what = '%s n_iter=%d row_parallel=%s' % (c['id'], n_iter, row_parallel)
        assert guards_intact(whole, n + ROOT_TAIL, G_OUT) and untouched(view[n:]), what + ': a row behind the rays was written'
        _ROOT_D[key] = view[:n].reshape(-1).cpu().numpy().copy()
    return _ROOT_D[key]


def assert_same_depths(a, b, inp, what):
    """int32 bits equal; on the rays whose bracket divides by zero (f_low == f_high) NaN in the same places and all other bits equal."""
    ff = np.array([k == 'ff' for k in inp['kinds']])
    ai, bi = a.view(np.int32), b.view(np.int32)
    assert np.array_equal(ai[~ff], bi[~ff]), '%s: %d rays differ, the first is ray %d: %r vs %r' % (
        what, int((ai != bi)[~ff].sum()), int(np.flatnonzero((ai != bi) & ~ff)[0]), a[(ai != bi) & ~ff][0], b[(ai != bi) & ~ff][0])
    na, nb = np.isnan(a[ff]), np.isnan(b[ff])
    assert np.array_equal(na, nb) and np.array_equal(ai[ff][~na], bi[ff][~na]), what + ': the degenerate rays differ'


@pytest.mark.parametrize('c', mc.H_CASES, ids=mc.case_id)
def test_root_finder_forms_agree_bit_for_bit(mods, cuda, c):
    """(a) + (b): at n_iter = 0, 1, 2, 3, 8 and 64 the feature-parallel and the row-parallel form write the same bits, and nothing but the
    n depths."""
    net, inp, pk, dev = root_device(c, mods, cuda)
    for k in mc.H_N_ITER:
        fp, rp = (root_depths(c, net, inp, pk, dev, mods, cuda, k, form) for form in ROOT_FORMS)
        assert_same_depths(fp, rp, inp, '%s n_iter=%d: feature-parallel vs row-parallel' % (c['id'], k))
    # the rays that are no division by zero stay finite to the end; d_low == d_high stays where it is
    last = root_depths(c, net, inp, pk, dev, mods, cuda, 64, False)
    kinds = np.array(inp['kinds'])
    # (a division by zero gives inf, and NaN from the first occupancy on -- unless the network is a ReLU one: v_max_f32 answers
    #  max(NaN, 0) = 0, the occupancy of the infinite point is a number and the depth stays inf)
    assert np.isfinite(last[kinds != 'ff']).all() and not np.isfinite(last[kinds == 'ff']).any()
    assert np.array_equal(last[kinds == 'dd'], inp['bracket'][0][kinds == 'dd'])
    x = inp['crossing']
    assert ((last[x] >= inp['bracket'][0][x]) & (last[x] <= inp['bracket'][1][x])).all(), c['id'] + ': a depth left its bracket'


@pytest.mark.parametrize('c', mc.H_CASES, ids=mc.case_id)
def test_root_finder_equals_the_stepwise_composition(mods, cuda, c):
    """(c): D[k], k = 0 .. 8, of both forms against the composition of kernels this suite gates elsewhere: psn_secant_step without an
    occupancy for the first estimate and query point, then per iteration psn_mlp_infer_pe on the query points and psn_secant_step with
    its occupancies.  Bit for bit: see the module docstring for the outcome on the device."""
    hip, _ = mods
    net, inp, pk, dev = root_device(c, mods, cuda)
    n = c['n']
    d_pred = torch.empty(n, device=cuda)
    d_low, d_high, f_low, f_high = (dev['bracket'][r].clone() for r in range(4))
    p_mid = torch.empty(n, 3, device=cuda)
    hip.secant_step(None, inp['tau'], d_pred, d_low, d_high, f_low, f_high, dev['origin'], dev['direction'], p_mid)
    steps = [d_pred.cpu().numpy().copy()]
    for k in range(mc.H_STEPWISE):
        occ = pk.on_points(p_mid, c['octaves'], c['pe_scale']).reshape(-1)
        hip.secant_step(occ, inp['tau'], d_pred, d_low, d_high, f_low, f_high, dev['origin'], dev['direction'], p_mid)
        steps.append(d_pred.cpu().numpy().copy())
    for k in range(mc.H_STEPWISE + 1):
        for form in ROOT_FORMS:
            got = root_depths(c, net, inp, pk, dev, mods, cuda, k, form)
            assert_same_depths(got, steps[k], inp, '%s D[%d] row_parallel=%s vs step by step' % (c['id'], k, form))


@pytest.mark.parametrize('c', mc.H_CASES, ids=mc.case_id)
def test_root_finder_iterates_vs_float64(mods, cuda, c):
    """(d): D[0] .. D[3] of both forms through mlp_cases.trace_check, the float64 check that follows the kernel's own iterates: D[0] has
    the bits of the float32 formula, every later iterate of a crossing ray lies within the allowance of an admissible float64
    candidate, and no (ray, iterate) pair is unchecked."""
    net, inp, pk, dev = root_device(c, mods, cuda)
    r_ref = mc.trace_check(net, inp, mc.root_find_definition(net, inp, mc.H_TRACE))
    assert r_ref['failures'] == 0 and r_ref['unchecked'] == 0 and r_ref['worst'] <= 0.5
    for form in ROOT_FORMS:
        D = [root_depths(c, net, inp, pk, dev, mods, cuda, k, form) for k in range(mc.H_TRACE + 1)]
        r = mc.trace_check(net, inp, D)
        name = mc.dispatch(c, net, row_parallel=form)['name']
        print('%s %-18s worst ratio %.3f at %s (float32 definition %.3f)' % (c['id'], name, r['worst'], r['where'], r_ref['worst']))
        assert r['first_equal'], '%s %s: D[0] is not the float32 secant estimate of the bracket' % (c['id'], name)
        assert r['failures'] == 0 and r['unchecked'] == 0, '%s %s: %r' % (c['id'], name, r)
        if r['worst'] > _WORST.get(name, (-1.0,))[0]:
            _WORST[name] = (r['worst'], r_ref['worst'], '%s ray %d D[%d]' % ((c['id'],) + (r['where'][0], r['where'][1] + 1)))


def _root_arg_setup(mods, cuda):
    c = [c for c in mc.H_CASES if c['id'] == 'H-rays65-depth4-skip8'][0]
    return (c,) + root_device(c, mods, cuda)


@pytest.mark.parametrize('a', mc.H_ARG_CASES, ids=mc.case_id)
def test_root_finder_argument_checks(mods, cuda, a):
    """PSN_E_ARG with the words of the check the case is built for, nothing launched (the thread's last path, zeroed by a call on no
    rays just before, stays zero) and the output untouched."""
    import ctypes
    import re
    hip, _ = mods
    c, net, inp, pk, dev = _root_arg_setup(mods, cuda)
    desc = type(pk.desc).from_buffer_copy(pk.desc)
    for k, v in a.get('desc', {}).items():
        setattr(desc, k, hip.W_BF16X2 if v == 'bf16x2' else v)
    if 'final_act' in a:
        desc.layers[desc.n_layers - 1].act = mc.ACT[a['final_act']]
    n = c['n']
    whole, view = nan_buffer(n, 1, cuda, G_OUT)
    args = lambda d, rays, n_iter: (ctypes.byref(d), pk.w.data_ptr(), pk.b.data_ptr(), dev['origin'].data_ptr(), dev['direction'].data_ptr(),
                                    dev['bracket'].data_ptr(), rays, float(inp['tau']), n_iter, c['octaves'], float(c['pe_scale']),
                                    view.data_ptr(), hip._stream())
    assert hip._lib.psn_root_find(*args(pk.desc, 0, 8)) == 0
    path = hip.PsnMlpPath()
    with pytest.raises(RuntimeError, match=re.escape(a['refusal'])):
        hip.root_find(desc, pk.w, pk.b, dev['origin'], dev['direction'], dev['bracket'], inp['tau'], a.get('n_iter', 8), c['octaves'],
                      c['pe_scale'], out=view.reshape(-1), path=path)
    hip._last_path(path)
    torch.cuda.synchronize()
    assert path.blocks == 0 and untouched(whole)


def test_root_finder_on_no_rays(mods, cuda):
    """n_rays = 0: PSN_OK, nothing launched, psn_mlp_last_path answers zeros (not the launch before), the output untouched; through
    the wrapper an empty result and a zeroed path."""
    import ctypes
    hip, _ = mods
    c, net, inp, pk, dev = _root_arg_setup(mods, cuda)
    n = c['n']
    whole, view = nan_buffer(n, 1, cuda, G_OUT)
    path = hip.PsnMlpPath()
    hip.root_find(pk.desc, pk.w, pk.b, dev['origin'], dev['direction'], dev['bracket'], inp['tau'], 1, c['octaves'], c['pe_scale'], path=path)
    assert path.blocks == (n + 15) // 16 and path.src == mc.SRC_ROOT
    rc = hip._lib.psn_root_find(ctypes.byref(pk.desc), pk.w.data_ptr(), pk.b.data_ptr(), dev['origin'].data_ptr(), dev['direction'].data_ptr(),
                                dev['bracket'].data_ptr(), 0, float(inp['tau']), 8, c['octaves'], float(c['pe_scale']), view.data_ptr(),
                                hip._stream())
    hip._last_path(path)
    torch.cuda.synchronize()
    assert rc == 0 and untouched(whole)
    assert (path.blocks, path.chain, path.width16, path.src, path.trim, path.from_a, path.x3) == (0, 0, 0, 0, 0, 0, 0)
    path.blocks = 7
    out = hip.root_find(pk.desc, pk.w, pk.b, dev['origin'][:0], dev['direction'][:0], dev['bracket'][:, :0].contiguous(), inp['tau'], 8,
                        c['octaves'], c['pe_scale'], path=path)
    assert out.shape == (0,) and path.blocks == 0


# --------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize('c', mc.ARG_CASES, ids=mc.case_id)
def test_argument_checks_refuse_and_launch_nothing(mods, cuda, c):
    """PSN_E_ARG with the message of the very check the case is built for; no output or dump buffer is written."""
    import re
    net = mc.build(c)
    pk = pack_net(net, mods, cuda)
    res = {}
    with pytest.raises(RuntimeError, match=re.escape(c['refusal'])):
        if c['kind'] == 'lean':
            run_lean(c, net, pk, mods, cuda, res=res)
        else:
            run_chain(c, net, pk, mods, cuda, res=res)
    torch.cuda.synchronize()
    assert res['bufs'] and all(untouched(w_) for w_, _, _ in res['bufs'])


def test_live_count_on_a_chain_launch_is_refused_by_the_library(mods, cuda):
    """A live count with no chain OPERAND at all still meets a chain launch when a program makes it one (HEAD): called through the
    C ABI directly, the `!chain` clause of the planner (csrc/mlp_infer.hip, mlp_infer_plan) answers PSN_E_ARG."""
    import ctypes
    hip, _ = mods
    n, row0 = 128, 64
    c = mc.chain('ARG-live-on-chain-abi', n=n, prog=('relu', 'head'), n_out=3)
    net = mc.build(c)
    pk = pack_net(net, mods, cuda)
    whole, out = nan_buffer(n, 3, cuda, G_OUT)
    dumps = [nan_buffer(n - row0, 256, cuda, G_OUT) for _ in range(2)]
    save = (ctypes.c_void_p * 2)(*[d.data_ptr() for _, d in dumps])
    ta, live = net.tab_a.to(cuda), torch.tensor([3.0], device=cuda)
    o, path = hip.PsnMlpLaunch(), hip.PsnMlpPath()
    o.tab_a, o.a_div, o.a_mod, o.b_div, o.b_mod = ta.data_ptr(), 1, n, 1, 1
    o.save_ptrs, o.save_row0, o.n_rows, o.out = ctypes.addressof(save), row0, n, out.data_ptr()
    o.live_count, o.live_period = live.data_ptr(), 64
    rc = hip._lib.psn_mlp_launch(ctypes.byref(pk.desc), pk.w.data_ptr(), pk.b.data_ptr(), ctypes.byref(o), ctypes.byref(path), hip._stream())
    assert rc != 0 and path.blocks == 0
    with pytest.raises(RuntimeError, match='mlp_infer_padded: needs the lean variant'):
        hip._check(rc, 'mlp_infer_padded')
    torch.cuda.synchronize()
    assert untouched(whole) and all(untouched(w_) for w_, _ in dumps)


def test_live_count_on_a_chain_launch_is_refused_by_the_wrapper(mods, cuda):
    """hip.mlp_infer states no rule of its own: a live count beside a chain operand (a mask) reaches the library, whose check (the
    test above) refuses it with the same words, and nothing is written."""
    hip, _ = mods
    c = mc.chain('ARG-live-on-chain', n=128, prog=('relu_mask', 'none'), n_out=3)
    net = mc.build(c)
    pk = pack_net(net, mods, cuda)
    whole, out = nan_buffer(128, 3, cuda, G_OUT)
    path = hip.PsnMlpPath()
    with pytest.raises(RuntimeError, match='mlp_infer_padded: needs the lean variant'):
        hip.mlp_infer(pk.desc, pk.w, pk.b, net.tab_a.to(cuda), 1, 128, None, 1, 1, 128, out=out, mask=[net.mask[0].to(cuda), None, None],
                      save_row0=64, live=(torch.tensor([3.0], device=cuda), 64), path=path)
    torch.cuda.synchronize()
    assert untouched(whole) and path.blocks == 0
