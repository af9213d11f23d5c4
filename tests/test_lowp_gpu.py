"""The reduced-precision inference family on the device, path by path, on the cases of tests/lowp_cases.py (whose exactness
conditions, coverage and sensitivity tests/test_lowp_cpu.py asserts without a GPU): the plain bf16 engine (csrc/mlp_infer_bf16.hip,
two-table and grouped form), the split-bf16 engine (csrc/mlp_infer_x3.hip: grouped form, occupancy form, ray-march sweep), the
packers of both and the PSN_W_BF16X2 weight stages of the fp32 engine (csrc/mlp_infer.hip).

The operands are chosen so that the arithmetic is exact (tests/lowp_cases.py): the launches are compared with the float64
reference with torch.equal, without a tolerance.  Only the output activations (sigmoid) and the random-weight check of family C
carry a bound: helpers.assert_vs_truth with mlp_cases.RTOL, 'max', the bound of the fp32 engine's suite.  Every output buffer starts
as NaNs of a fixed bit pattern inside a larger buffer: what a launch must not write keeps its bits.

Measured on an MI355X.  Every exact comparison holds bit for bit -- also B1: the MFMA's fp32 accumulation of non-overlapping
bf16 pieces is exact (worst distance from the float64 reference over all B1 cases: 0 ulp, so the assertion is torch.equal), the occupancy
form of the split engine equals the exact engine on selection weights including its softplus layers, and the PSN_W_BF16X2 stages
round as their header comment says (the model of lowp_cases.x3dot fits).  Worst r_hip per path, in units of the bound:
    path                   r_hip   r_ref   worst tensor
    bf16/two/sigmoid       0.003   0.003   A1-sigmoid
    bf16/two/occ           0.000   0.000   A1-occ            (integer logits: the occupancies sit at 0 or 1)
    bf16/grouped/sigmoid   0.003   0.003   A1-grouped-sigmoid
    bf16/grouped/occ       0.003   0.003   A1-grouped-occ
    bf16x2/chain           0.394   0.427   C2-chain dump3    (logit 0.149, features 0.335, dumps 0.011 / 0.111 / 0.249 / 0.394)
    bf16x2/occupancy       0.092   0.084   C2-occupancy
134 tests, 1.6 s of wall time for the module.

What the outputs observe: output 0 of a split-engine case reads a feature that differs from row to row; the other outputs of the
32-output cases read, on purpose, one constant feature of EVERY hidden layer (its bias k-step, from the stream or -- input layers --
from V) and the per-group feature w x_g + b of every input layer, handed on to the final layer (lowp_cases.build_x3_net; the
B2-bias-layer networks do the same for the occupancy form, one hidden layer per network).  tests/test_lowp_cpu.py asserts that
every hidden layer's bias changes an output and that a bias k-step without its lo piece, the wrong layer's bias k-step, group
0's V row and the first input layer's tables in place of the second each change one.

Finding of this suite (fixed in psnerf_amd/hip.py, test_zero_size_launches_return_cleanly and the last lines of
test_x3_engine_refuses_bad_arguments_and_launches_nothing kept): a launch of no rows through the Python binding -- mlp_infer_bf16,
mlp_infer_bf16_grouped, mlp_infer_x3_grouped, mlp_infer_x3_occ with an empty table or point set -- did not return an empty result
but raised "null pointer": an empty tensor has no device pointer, and the library checks its pointers before it looks at the row
count.  The four wrappers now validate their tensors as for any launch and then return the empty result without a call, as
mlp_infer_pe always did; the library itself (called with valid pointers and a zero count) returns cleanly and writes nothing,
which the same tests assert through the C ABI for all five launches.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import lowp_cases as lc
from tests import mlp_cases as mc
from tests.helpers import assert_vs_truth, truth_ratios

pytestmark = pytest.mark.gpu
_WORST = {}      # path -> (worst r_hip, r_ref there, case)
NAN_BITS = lc.NAN_BITS
G_OUT = lc.GUARD
OUT_CODE = dict(none=0, sigmoid=1, occ=2)


@pytest.fixture(scope='module', autouse=True)
def _report():
    import time
    t0 = time.time()
    yield
    if _WORST:
        print('\n==== reduced-precision engines: worst r_hip per path (r_ref in the same tensor), in units of the bound ====')
        for name, (rh, rr, where) in sorted(_WORST.items()):
            print('%-26s r_hip %6.3f  r_ref %6.3f  (%s)' % (name, rh, rr, where))
    print('module wall time %.1f s' % (time.time() - t0))


@pytest.fixture(scope='module')
def mods(cuda):
    from psnerf_amd import hip, fused
    return hip, fused


def nan_buffer(rows, cols, cuda, guard=G_OUT):
    """(whole, view): ``rows`` x ``cols`` floats of NAN_BITS with ``guard`` rows of the same in front and behind."""
    whole = torch.full((rows + 2 * guard, cols), NAN_BITS, dtype=torch.int32, device=cuda).view(torch.float32)
    return whole, whole[guard:guard + rows]


def untouched(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


def guards_intact(whole, rows, guard=G_OUT):
    return untouched(whole[:guard]) and untouched(whole[guard + rows:])


def record(path, what, got, truth, ref):
    """The figures first (worst distance from the float64 truth in units of the bound: the launch, the CPU float32 reference
    arithmetic), then the assertion of helpers.assert_vs_truth."""
    got = got.detach().cpu().numpy()
    assert got.shape == tuple(truth.shape), '%s: shape %s vs %s' % (what, got.shape, tuple(truth.shape))
    r_hip, r_ref, _, _, _ = truth_ratios(got, ref.numpy(), truth.numpy(), mc.RTOL, 'max')
    rh, rr = float(r_hip.max()), float(r_ref.max())
    print('%s r_hip %.3f r_ref %.3f' % (what, rh, rr))
    if rh > _WORST.get(path, (-1.0,))[0]:
        _WORST[path] = (rh, rr, what)
    assert_vs_truth(what, got, ref.numpy(), truth.numpy(), mc.RTOL, 'max')


def same_bits16(got, ref):
    return np.array_equal(got.contiguous().view(torch.int16).cpu().numpy().reshape(-1), ref)


# --------------------------------------------------------------------------- A: the plain bf16 engine
def pack_bf16(net, c, mods, cuda, out_act):
    hip, fused = mods
    Ws, bs = [w.to(cuda) for w in net.Ws], [b.to(cuda) for b in net.bs]
    f = fused.pack_relu_mlp_bf16_grouped if c['form'] == 'grouped' else fused.pack_relu_mlp_bf16
    return f(Ws, bs, net.din_a, net.din_b, net.skip_at, OUT_CODE[out_act])


def run_bf16(net, c, pk, cuda):
    n = c['n']
    whole, out = nan_buffer(n, net.n_out, cuda)
    ta = net.tab_a.to(cuda).to(torch.bfloat16)
    if c['form'] == 'grouped':
        pk(ta, net.tab_b.to(cuda), out=out)
    else:
        a_div, a_mod, b_div, b_mod = c['maps']
        tb = None if net.tab_b is None else net.tab_b.to(cuda).to(torch.bfloat16)
        pk(ta, n, a_div=a_div, a_mod=a_mod, tab_b=tb, b_div=b_div, b_mod=b_mod, out=out)
    assert guards_intact(whole, n), '%s: a guard row was written' % c['id']
    return out


@pytest.mark.parametrize('c', lc.A_CASES, ids=lc.case_id)
def test_bf16_engine_is_exact(mods, cuda, c):
    """A1 (integer networks) and A2 (rounding probes), both forms: the logits equal the float64 reference bit for bit; a sigmoid /
    occupancy output is then held to the fp32 engine's bound against the float64 activation of the exact logit."""
    net, ref = lc.reference_bf16(c)
    want = ref['logit'].float()
    got = run_bf16(net, c, pack_bf16(net, c, mods, cuda, 'none'), cuda)
    bad = (got.cpu() != want)
    assert torch.equal(got.cpu(), want), '%s: %d of %d logits differ, first at %s: got %r, want %r' % (
        c['id'], int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got.cpu()[bad][0]), float(want[bad][0]))
    if c['out_act'] != 'none':
        truth, ref32 = lc.activated(ref['logit'], c['out_act'])
        act = run_bf16(net, c, pack_bf16(net, c, mods, cuda, c['out_act']), cuda)
        record('bf16/%s/%s' % (c['form'], c['out_act']), c['id'], act, truth, ref32)


def test_bf16_group_bias_rows_arrive_exactly(mods, cuda):
    """The V rows of a grouped probe case, W_b x_g + b formed by the fp32 GEMM, equal the reference's bit for bit: the probe values
    reach psn_lowp_pack_bias as the reference states them."""
    hip, _ = mods
    c = [x for x in lc.A2_CASES if x['form'] == 'grouped'][1]
    net, ref = lc.reference_bf16(c)
    pk = pack_bf16(net, c, mods, cuda, 'none')
    V = hip.gemm(net.tab_b.to(cuda), pk.wb_t, bias=pk.b_in, epi=hip.EPI_BIAS).cpu()
    assert pk.n_in == len(ref['V']) == 2
    for i, v in enumerate(ref['V']):
        assert torch.equal(V[:, 256 * i:256 * (i + 1)], v)


# --------------------------------------------------------------------------- B1: the split engine, grouped form
@pytest.mark.parametrize('c', lc.B1_CASES, ids=lc.case_id)
def test_x3_grouped_propagates_full_mantissas_exactly(mods, cuda, c):
    hip, fused = mods
    net, ref = lc.reference_x3(c)
    Ws, bs = [w.to(cuda) for w in net.Ws], [b.to(cuda) for b in net.bs]
    pk = fused.pack_relu_mlp_x3_grouped(Ws, bs, net.din_a, net.din_b, net.skip_at)
    ta, tb = net.tab_a.to(cuda), net.tab_b.to(cuda)
    # the init tables are what the reference says: one exact product per element
    U = hip.gemm(ta, pk.init_wa, trans_b=True).cpu()
    V = hip.gemm(tb, pk.init_wb, trans_b=True, bias=pk.init_bias, epi=hip.EPI_BIAS).cpu()
    for i, (u, v) in enumerate(zip(ref['U'], ref['V'])):
        assert torch.equal(U[:, 256 * i:256 * (i + 1)], u) and torch.equal(V[:, 256 * i:256 * (i + 1)], v)
    n = c['n']
    whole, out = nan_buffer(n, net.n_out, cuda)
    pk(ta, tb, out=out)
    assert guards_intact(whole, n)
    d = lc.ulp_distance(out.cpu(), ref['out'])
    print('%s: worst distance %.2f ulp' % (c['id'], d))
    bad = (out.cpu() != ref['out'].float()).any(0).nonzero().reshape(-1).tolist()
    assert torch.equal(out.cpu(), ref['out'].float()), '%s: worst distance %.2f ulp, outputs %s differ (bias tracers: %s)' % (c['id'], d, bad, net.traced)


# --------------------------------------------------------------------------- B3: the packers
def _views(item, cuda):
    store, view = lc.pack_matrix(item)
    v = store.to(cuda)[:, item['col0']:item['col0'] + item['cols']]
    assert v.stride(0) == item['cols'] + item['ldw_extra'] and v.stride(1) == 1
    return v, view.numpy()


def _bf16_guarded(n, cuda):
    whole = torch.full((n + 32,), 0x7FC1, dtype=torch.int16, device=cuda).view(torch.bfloat16)
    return whole, whole[16:16 + n]


def _guard16(whole, n):
    w = whole.view(torch.int16)
    return bool((w[:16] == 0x7FC1).all()) and bool((w[16 + n:] == 0x7FC1).all())


@pytest.mark.parametrize('item', lc.PACK_ITEMS, ids=lc.case_id)
def test_bf16_packer_equals_layout_model(mods, cuda, item):
    hip, _ = mods
    v, W = _views(item, cuda)
    n = item['n_ks'] * item['n_ot'] * 512
    whole, dst = _bf16_guarded(n, cuda)
    hip.lowp_pack(v, item['permuted'], item['n_ot'], item['ks0'], item['n_ks'], dst, planes=1)
    assert same_bits16(dst, lc.pack_bf16_reference(W, item['permuted'], item['n_ot'], item['ks0'], item['n_ks'])) and _guard16(whole, n)


@pytest.mark.parametrize('item', lc.PACK_ITEMS, ids=lc.case_id)
def test_x3_packer_planes_sum_to_the_source(mods, cuda, item):
    hip, _ = mods
    v, W = _views(item, cuda)
    n = item['n_ks'] * item['n_ot'] * 3 * 512
    whole, dst = _bf16_guarded(n, cuda)
    hip.lowp_pack(v, item['permuted'], item['n_ot'], item['ks0'], item['n_ks'], dst, planes=3)
    assert _guard16(whole, n)
    p = dst.float().cpu().view(item['n_ks'], item['n_ot'], 3, 64, 8)
    src = torch.from_numpy(lc.pack_source(W, item['permuted'], item['n_ot'], item['ks0'], item['n_ks']))
    assert torch.equal((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2], src)      # exact, and 0 where the source was zero-extended
    assert same_bits16(dst, lc.pack_x3_reference(W, item['permuted'], item['n_ot'], item['ks0'], item['n_ks']))


@pytest.mark.parametrize('n', lc.BIAS_ROWS)
def test_bias_step_packers_equal_layout_model(mods, cuda, n):
    hip, _ = mods
    V = lc.bias_matrix(n)
    for pieces in (2, 3):
        whole, dst = _bf16_guarded(n * 4096, cuda)
        hip.lowp_pack_bias(V.to(cuda), pieces, dst.view(n, 4096))
        assert same_bits16(dst, lc.bias_step_reference(V, pieces)) and _guard16(whole, n * 4096), pieces


# --------------------------------------------------------------------------- argument checks
def _refused(hip, rc, what, message):
    assert rc != 0
    with pytest.raises(RuntimeError, match=re.escape(message)):
        hip._check(rc, what)


def _desc_copy(hip, d, **kw):
    e = hip.PsnBf16Desc()
    e.n_hidden, e.n_out, e.out_act = d.n_hidden, d.n_out, d.out_act
    for i in range(len(d.has_in)):
        e.has_in[i] = d.has_in[i]
    for k, v in kw.items():
        if k == 'has_in0':
            e.has_in[0] = v
        else:
            setattr(e, k, v)
    return e


def test_bf16_engine_refuses_bad_arguments_and_launches_nothing(mods, cuda):
    hip, _ = mods
    c = lc.two('ARG-bf16', n=65)
    net = lc.build_bf16(c)
    pk = pack_bf16(net, c, mods, cuda, 'none')
    cg = lc.grouped('ARG-bf16-grouped', rpg=33, groups=3)
    netg = lc.build_bf16(cg)
    pkg = pack_bf16(netg, cg, mods, cuda, 'none')
    gb = pkg.group_bias(netg.tab_b.to(cuda))
    whole, out = nan_buffer(99, 32, cuda)
    ta = torch.zeros(20 * 64 + 8, device=cuda, dtype=torch.bfloat16)
    tab, tab_odd = ta[:19 * 64].view(19, 64), ta[1:1 + 19 * 64]     # the second: 2 bytes off a 16-byte boundary
    assert tab.data_ptr() % 16 == 0 and tab_odd.data_ptr() % 16 == 2
    st = hip._stream()

    def two_(desc=pk.desc, tab_a=tab.data_ptr(), a_div=1, tab_b=tab.data_ptr()):
        return hip._lib.psn_mlp_infer_bf16(ctypes.byref(desc), pk.w.data_ptr(), pk.final_bias.data_ptr(), tab_a, a_div, 19, tab_b, 19, 4, 65,
                                           out.data_ptr(), st)

    def grouped_(desc):
        return hip._lib.psn_mlp_infer_bf16_grouped(ctypes.byref(desc), pkg.w.data_ptr(), pkg.final_bias.data_ptr(), tab.data_ptr(), 19, gb.data_ptr(), 3,
                                                   out.data_ptr(), st)
    for kw, msg in ((dict(n_out=0), 'n_out=0'), (dict(n_out=33), 'n_out=33'), (dict(n_hidden=0), 'n_hidden=0'), (dict(n_hidden=13), 'n_hidden=13'),
                    (dict(has_in0=0), 'layer 0 must read the input block')):
        _refused(hip, two_(desc=_desc_copy(hip, pk.desc, **kw)), 'mlp_infer_bf16', 'mlp_infer_bf16: ' + msg)
        _refused(hip, grouped_(_desc_copy(hip, pkg.desc, **kw)), 'mlp_infer_bf16_grouped', 'mlp_infer_bf16_grouped: ' + msg)
    _refused(hip, two_(tab_a=tab_odd.data_ptr()), 'mlp_infer_bf16', 'buffers must be 16-byte aligned')
    _refused(hip, two_(tab_b=tab_odd.data_ptr()), 'mlp_infer_bf16', 'buffers must be 16-byte aligned')
    _refused(hip, two_(a_div=0), 'mlp_infer_bf16', 'bad index map')
    with pytest.raises(RuntimeError, match='tab_a: must be bfloat16'):
        pk(torch.zeros(19, 64, device=cuda), 65, a_div=1, a_mod=19, tab_b=tab, b_div=19, b_mod=4, out=out[:65, :3].contiguous())
    with pytest.raises(RuntimeError, match='tab_a: must be bfloat16'):
        pkg(torch.zeros(19, 64, device=cuda), netg.tab_b.to(cuda))
    # ... and a launch of no rows validates its tables like any other
    with pytest.raises(RuntimeError, match='tab_a: must be bfloat16'):
        pk(torch.zeros(19, 64, device=cuda), 0, a_div=1, a_mod=19, tab_b=tab, b_div=19, b_mod=4)
    with pytest.raises(RuntimeError, match='tab_a: must be bfloat16'):
        pkg(torch.zeros(0, 64, device=cuda), netg.tab_b.to(cuda))
    torch.cuda.synchronize()
    assert untouched(whole)
    # the refusals left the engine usable: the same calls with good arguments run
    assert two_() == 0 and grouped_(pkg.desc) == 0
    torch.cuda.synchronize()
    assert not untouched(out.reshape(-1)[:171])


def pkg_rows0(mods, cuda):
    """Shape of the grouped form's result for a table A without rows (through the wrapper)."""
    cg = lc.grouped('ARG-zero-rows', rpg=33, groups=3)
    netg = lc.build_bf16(cg)
    pkg = pack_bf16(netg, cg, mods, cuda, 'none')
    return tuple(pkg(torch.zeros(0, 64, device=cuda, dtype=torch.bfloat16), netg.tab_b.to(cuda)).shape)


def test_zero_size_launches_return_cleanly(mods, cuda):
    hip, fused = mods
    c = lc.two('ARG-zero', n=65)
    net = lc.build_bf16(c)
    pk = pack_bf16(net, c, mods, cuda, 'none')
    whole, out = nan_buffer(8, 3, cuda)
    ta = net.tab_a.to(cuda).to(torch.bfloat16)
    assert pk(ta, 0, a_div=1, a_mod=ta.shape[0], tab_b=ta, b_div=1, b_mod=1).shape == (0, 3)       # the wrapper: an empty result
    assert pkg_rows0(mods, cuda) == (0, 3)
    assert hip._lib.psn_mlp_infer_bf16(ctypes.byref(pk.desc), pk.w.data_ptr(), pk.final_bias.data_ptr(), ta.data_ptr(), 1, ta.shape[0], ta.data_ptr(), 1, 1,
                                       0, out.data_ptr(), hip._stream()) == 0
    cg = lc.grouped('ARG-zero-grouped', rpg=33, groups=3)
    netg = lc.build_bf16(cg)
    pkg = pack_bf16(netg, cg, mods, cuda, 'none')
    gb = pkg.group_bias(netg.tab_b.to(cuda))
    st = hip._stream()
    for rows, groups in ((0, 3), (33, 0), (0, 0)):
        assert hip._lib.psn_mlp_infer_bf16_grouped(ctypes.byref(pkg.desc), pkg.w.data_ptr(), pkg.final_bias.data_ptr(), ta.data_ptr(), rows,
                                                   gb.data_ptr(), groups, out.data_ptr(), st) == 0
    cx = lc.x3case('ARG-zero-x3')
    netx = lc.build_x3_net(cx)
    pkx = fused.pack_relu_mlp_x3_grouped([w.to(cuda) for w in netx.Ws], [b.to(cuda) for b in netx.bs], 63, 63, netx.skip_at)
    U, V = torch.zeros(33, 512, device=cuda), torch.zeros(3, 512, device=cuda)
    for rows, groups in ((0, 3), (33, 0), (0, 0)):
        assert hip._lib.psn_mlp_infer_x3_grouped(ctypes.byref(pkx.desc), pkx.w.data_ptr(), pkx.bias_steps.data_ptr(), pkx.final_bias.data_ptr(),
                                                 U.data_ptr(), rows, V.data_ptr(), groups, out.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert untouched(whole)


# --------------------------------------------------------------------------- B2: occupancy form and sweep against the exact engine
def pack_occ(net, mods, cuda):
    hip, fused = mods
    Ws, bs = [w.to(cuda) for w in net.Ws], [b.to(cuda) for b in net.bs]
    # the fold of 1 / sqrt 2 into the skip layer leaves powers of two on the device as it does on the CPU
    w = (Ws[net.skips[0]] * (1.0 / 2.0 ** 0.5)).cpu()
    assert torch.equal(lc.bf16(w), w)
    return fused.pack_geo_occupancy_x3(Ws, bs, net.skips, lc.OCC_DPE), fused.pack_geo_occupancy(Ws, bs, net.skips, lc.OCC_DPE)


def _diff(a, b):
    bad = a != b
    return '%d of %d entries differ, worst |a - b| %.3e' % (int(bad.sum()), bad.numel(), float((a - b).abs().max()) if bad.numel() else 0.0)


@pytest.mark.parametrize('c', lc.B2_POINT_CASES + lc.B2_BIAS_CASES, ids=lc.case_id)
def test_x3_occupancy_equals_exact_engine_on_selection_weights(mods, cuda, c):
    net = lc.build_occ_net(c)
    pk3, pk32 = pack_occ(net, mods, cuda)
    assert pk3.skip_layer == c['skip'] and pk3.pe_first == lc.OCC_PE_FIRST
    n = c['n']
    pts = net.points.to(cuda).contiguous()
    whole, out = nan_buffer(n, 1, cuda)
    pk3.on_points(pts, lc.OCC_OCTAVES, lc.OCC_SCALE, out=out)
    want = pk32.on_points(pts, lc.OCC_OCTAVES, lc.OCC_SCALE)
    assert guards_intact(whole, n) and out.shape == want.shape
    assert torch.equal(out, want), '%s: %s' % (c['id'], _diff(out, want))
    if c['trace'] is None:
        assert n < 31 or want.unique().numel() > 8
    else:   # the bias of hidden layer c['trace'], handed on: the same for every point, and an occupancy away from 0 and 1
        assert want.unique().numel() == 1 and 0.02 < float(want[0]) < 0.98


@pytest.mark.parametrize('count', lc.OCC_COUNTS)
@pytest.mark.parametrize('scatter', (False, True), ids=('dense', 'scatter'))
def test_x3_occupancy_indirect_form(mods, cuda, count, scatter):
    """n_rows_dev below, at and above the capacity; out_rows scatters into a guarded buffer; rows behind the count keep their bits."""
    c = lc.occ('B2-indirect', n=lc.OCC_CAPACITY)
    net = lc.build_occ_net(c)
    pk3, pk32 = pack_occ(net, mods, cuda)
    Q = lc.OCC_CAPACITY
    pts = net.points.to(cuda).contiguous()
    want = pk32.on_points(pts, lc.OCC_OCTAVES, lc.OCC_SCALE)
    cnt = min(count, Q)
    count_dev = torch.tensor([count], dtype=torch.int64, device=cuda)
    if not scatter:
        whole, out = nan_buffer(Q, 1, cuda)
        pk3.on_points(pts, lc.OCC_OCTAVES, lc.OCC_SCALE, out=out, n_rows_dev=count_dev)
        assert guards_intact(whole, Q) and untouched(out[cnt:])
        got = out[:cnt]
    else:
        R = lc.OCC_SCATTER_ROWS
        perm = torch.randperm(R, generator=torch.Generator().manual_seed(count))[:Q].to(cuda)
        whole, out = nan_buffer(R, 1, cuda)
        pk3.on_points(pts, lc.OCC_OCTAVES, lc.OCC_SCALE, out=out, n_rows_dev=count_dev, out_rows=perm)
        named = torch.zeros(R, dtype=torch.bool, device=cuda)
        named[perm[:cnt]] = True
        assert guards_intact(whole, R) and untouched(out[~named]), 'an entry that no out_rows names was written'
        got = out[perm[:cnt]]
    assert torch.equal(got, want[:cnt]), _diff(got, want[:cnt])


def _sweep_x3(hip, pk3, s, n_rays, n_steps, cuda, early_exit):
    """psn_march_sweep_x3 through the C ABI into a NaN-patterned, guarded occupancy buffer -> (whole, occ, skip flags or None)."""
    whole, occ = nan_buffer(n_rays, n_steps, cuda)
    skip = torch.zeros(n_rays, dtype=torch.int32, device=cuda) if early_exit else None
    dv = lambda k: s[k].to(cuda).contiguous()
    keep = [dv(k) for k in ('origin', 'direction', 'far', 'u', 'omu')]
    rc = hip._lib.psn_march_sweep_x3(ctypes.byref(pk3.desc), pk3.w.data_ptr(), pk3.bias_steps.data_ptr(), pk3.final_bias.data_ptr(),
                                     keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(),
                                     float(s['near']), n_rays, n_steps, 0.5, lc.OCC_OCTAVES, lc.OCC_SCALE, pk3.skip_layer, pk3.pe_first,
                                     None if skip is None else skip.data_ptr(), occ.data_ptr(), None, hip._stream())
    hip._check(rc, 'march_sweep_x3')
    torch.cuda.synchronize()
    return whole, occ, skip


@pytest.mark.parametrize('n_steps', lc.SWEEP_STEPS)
@pytest.mark.parametrize('n_rays', lc.SWEEP_RAYS)
def test_x3_march_sweep(mods, cuda, n_rays, n_steps):
    """Full sweep = on_points of psn_sample_points' points, bit for bit, and equal to the exact engine's sweep; with early exit every
    entry up to and including the pair of the first sign change equals the full sweep, every other entry equals it or keeps its
    NaN pattern, and the flag names the first block whose workgroup sees a change."""
    hip, _ = mods
    net = lc.build_occ_net(lc.occ('B2-sweep', sweep=True))
    pk3, pk32 = pack_occ(net, mods, cuda)
    s = lc.sweep_rays(n_rays, n_steps)
    whole, full, _ = _sweep_x3(hip, pk3, s, n_rays, n_steps, cuda, False)
    assert guards_intact(whole, n_rays)
    dv = lambda k: s[k].to(cuda).contiguous()
    pts = torch.empty(n_rays, n_steps, 3, device=cuda)
    hip.sample_points(dv('origin'), dv('direction'), dv('far'), pts, False, s['near'], (dv('u'), dv('omu')))
    direct = pk3.on_points(pts.view(-1, 3), lc.OCC_OCTAVES, lc.OCC_SCALE)
    assert torch.equal(full.reshape(-1, 1), direct), _diff(full.reshape(-1, 1), direct)
    exact = pk32.on_points(pts.view(-1, 3), lc.OCC_OCTAVES, lc.OCC_SCALE)
    assert torch.equal(direct, exact), _diff(direct, exact)
    # the wrapper's own launches: the same bits
    occ_w, skip_w = pk3.march_sweep(dv('origin'), dv('direction'), dv('far'), dv('u'), dv('omu'), s['near'], n_steps, 0.5, lc.OCC_OCTAVES,
                                    lc.OCC_SCALE, early_exit=False)
    assert skip_w is None and torch.equal(occ_w, full)
    idx, blk = lc.first_change(full.cpu() - 0.5)
    kinds = s['kind']
    assert bool((idx[kinds == 1] == 0).all()) and bool((idx[kinds == 2] == -1).all()) and bool((idx[kinds == 3] > 0).all())
    assert bool((idx[kinds == 0] == (127 if n_steps == 256 else n_steps - 2)).all())
    whole, early, skip = _sweep_x3(hip, pk3, s, n_rays, n_steps, cuda, True)
    assert guards_intact(whole, n_rays)
    e, f = early.cpu().view(torch.int32), full.cpu().view(torch.int32)
    for r in range(n_rays):
        upto = n_steps if idx[r] < 0 else int(idx[r]) + 2
        if blk[r] >= 0:
            upto = max(upto, 128 * (int(blk[r]) + 1))    # the flagged block itself is complete
        else:
            upto = n_steps                                # no workgroup sees a change: nothing may be skipped
        assert torch.equal(e[r, :upto], f[r, :upto]), 'ray %d (kind %d)' % (r, int(kinds[r]))
        rest = e[r, upto:]
        assert bool(((rest == f[r, upto:]) | (rest == NAN_BITS)).all()), 'ray %d: a skipped entry lost its NaN pattern' % r
        assert int(skip[r]) == (0 if blk[r] < 0 else 0x7fffffff - int(blk[r]))


def test_x3_engine_refuses_bad_arguments_and_launches_nothing(mods, cuda):
    hip, fused = mods
    cx = lc.x3case('ARG-x3')
    netx = lc.build_x3_net(cx)
    pkx = fused.pack_relu_mlp_x3_grouped([w.to(cuda) for w in netx.Ws], [b.to(cuda) for b in netx.bs], 63, 63, netx.skip_at)
    net = lc.build_occ_net(lc.occ('ARG-occ', n=33))
    pk3, _ = pack_occ(net, mods, cuda)
    whole, out = nan_buffer(300, 32, cuda)
    buf = torch.zeros(40 * 512 + 8, device=cuda)
    U, V, U_odd = buf[:33 * 512].view(33, 512), buf[33 * 512:36 * 512].view(3, 512), buf[1:1 + 33 * 512]
    assert U.data_ptr() % 16 == 0 and V.data_ptr() % 16 == 0 and U_odd.data_ptr() % 16 == 4
    pts = net.points.to(cuda).contiguous()
    s = lc.sweep_rays(3, 128)
    ray = [s[k].to(cuda).contiguous() for k in ('origin', 'direction', 'far', 'u', 'omu')]
    st = hip._stream()

    def grouped_(desc=pkx.desc, u=U.data_ptr(), v=V.data_ptr()):
        return hip._lib.psn_mlp_infer_x3_grouped(ctypes.byref(desc), pkx.w.data_ptr(), pkx.bias_steps.data_ptr(), pkx.final_bias.data_ptr(), u, 33, v, 3,
                                                 out.data_ptr(), st)

    def occ_(desc=pk3.desc, octaves=lc.OCC_OCTAVES, skip_layer=pk3.skip_layer, pe_first=pk3.pe_first):
        return hip._lib.psn_mlp_infer_x3_occ(ctypes.byref(desc), pk3.w.data_ptr(), pk3.bias_steps.data_ptr(), pk3.final_bias.data_ptr(), pts.data_ptr(), 33,
                                             None, None, octaves, lc.OCC_SCALE, skip_layer, pe_first, out.data_ptr(), st)

    def sweep_(n_steps=128, octaves=lc.OCC_OCTAVES, skip_layer=pk3.skip_layer, pe_first=pk3.pe_first, w=pk3.w.data_ptr()):
        return hip._lib.psn_march_sweep_x3(ctypes.byref(pk3.desc), w, pk3.bias_steps.data_ptr(), pk3.final_bias.data_ptr(),
                                           ray[0].data_ptr(), ray[1].data_ptr(), ray[2].data_ptr(), ray[3].data_ptr(), ray[4].data_ptr(), 0.25, 3, n_steps,
                                           0.5, octaves, lc.OCC_SCALE, skip_layer, pe_first, None, out.data_ptr(), None, st)
    _refused(hip, grouped_(desc=_desc_copy(hip, pkx.desc, n_hidden=1)), 'mlp_infer_x3_grouped', 'mlp_infer_x3_grouped: n_hidden=1')
    _refused(hip, occ_(desc=_desc_copy(hip, pk3.desc, n_hidden=1)), 'mlp_infer_x3_occ', 'mlp_infer_x3_occ: n_hidden=1')
    _refused(hip, grouped_(u=U_odd.data_ptr()), 'mlp_infer_x3_grouped', 'buffers must be 16-byte aligned')
    _refused(hip, grouped_(v=U_odd.data_ptr()), 'mlp_infer_x3_grouped', 'buffers must be 16-byte aligned')
    _refused(hip, occ_(octaves=8), 'mlp_infer_x3_occ', '8 octaves do not fit 48 encoding columns')
    _refused(hip, sweep_(octaves=8), 'march_sweep_x3', '8 octaves do not fit 48 encoding columns')
    _refused(hip, occ_(skip_layer=pk3.desc.n_hidden), 'mlp_infer_x3_occ', 'skip_layer=%d' % pk3.desc.n_hidden)
    _refused(hip, sweep_(skip_layer=pk3.desc.n_hidden), 'march_sweep_x3', 'skip_layer=%d' % pk3.desc.n_hidden)
    _refused(hip, occ_(pe_first=191), 'mlp_infer_x3_occ', 'pe_first=191')
    _refused(hip, sweep_(pe_first=191), 'march_sweep_x3', 'pe_first=191')
    _refused(hip, sweep_(n_steps=200), 'march_sweep_x3', 'n_steps=200 must be a multiple of 128')
    _refused(hip, sweep_(n_steps=64), 'march_sweep_x3', 'n_steps=64 must be a multiple of 128')
    assert pk3.w.data_ptr() % 16 == 0     # ... and 2 bytes off that boundary: refused like its siblings' streams, before any launch
    _refused(hip, sweep_(w=pk3.w.data_ptr() + 2), 'march_sweep_x3', 'buffers must be 16-byte aligned')
    torch.cuda.synchronize()
    assert untouched(whole)
    assert grouped_() == 0 and occ_() == 0 and sweep_() == 0     # the same calls with good arguments run
    torch.cuda.synchronize()
    assert not untouched(out.reshape(-1)[:33])
    # zero rows through the wrappers: an empty result, nothing launched
    assert pk3.on_points(pts[:0], lc.OCC_OCTAVES, lc.OCC_SCALE).shape == (0, 1)
    assert hip.mlp_infer_x3_grouped(pkx.desc, pkx.w, pkx.bias_steps, pkx.final_bias, U[:0], V).shape == (0, netx.n_out)
    with pytest.raises(RuntimeError, match='U: must be a HIP device tensor'):      # validated like a launch with rows
        hip.mlp_infer_x3_grouped(pkx.desc, pkx.w, pkx.bias_steps, pkx.final_bias, torch.zeros(0, 512), V)
    with pytest.raises(RuntimeError, match='points: must be float32'):
        pk3.on_points(pts[:0].double(), lc.OCC_OCTAVES, lc.OCC_SCALE)
    # ... and the library itself, with valid pointers and a zero count
    whole0, out0 = nan_buffer(8, 1, cuda)
    assert hip._lib.psn_mlp_infer_x3_occ(ctypes.byref(pk3.desc), pk3.w.data_ptr(), pk3.bias_steps.data_ptr(), pk3.final_bias.data_ptr(), pts.data_ptr(), 0,
                                         None, None, lc.OCC_OCTAVES, lc.OCC_SCALE, pk3.skip_layer, pk3.pe_first, out0.data_ptr(), st) == 0
    assert hip._lib.psn_march_sweep_x3(ctypes.byref(pk3.desc), pk3.w.data_ptr(), pk3.bias_steps.data_ptr(), pk3.final_bias.data_ptr(),
                                       ray[0].data_ptr(), ray[1].data_ptr(), ray[2].data_ptr(), ray[3].data_ptr(), ray[4].data_ptr(), 0.25, 0, 128,
                                       0.5, lc.OCC_OCTAVES, lc.OCC_SCALE, pk3.skip_layer, pk3.pe_first, None, out0.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert untouched(whole0)


# --------------------------------------------------------------------------- C: PSN_W_BF16X2 weight stages of the fp32 engine
def _run_c1(c, net, pk, ta, tb, mods, cuda, order=None):
    hip, _ = mods
    n = c['n']
    a_div, a_mod, b_div, b_mod = c['maps']
    whole, out = nan_buffer(n, net.n_out, cuda)
    kw = {}
    if c['live'] is not None:
        kw = dict(live=(torch.tensor([float(c['live'])], device=cuda), c['period']), save_row0=c['save_row0'])
    path = hip.PsnMlpPath()
    call = lambda: pk(ta, n, a_div=a_div, a_mod=a_mod, tab_b=tb, b_div=b_div, b_mod=b_mod, out=out, path=path, **kw)
    if order is None:
        call()
    else:
        with hip.block_order(order):
            call()
    assert guards_intact(whole, n)
    # the lean engine, on split-bf16 stages exactly when the pack holds them
    assert path.blocks > 0 and not path.chain and path.x3 == int(pk.desc.w_format == hip.W_BF16X2)
    return out


@pytest.mark.parametrize('c', lc.C1_CASES, ids=lc.case_id)
def test_bf16x2_stages_on_selection_weights_equal_fp32_stages_on_split_inputs(mods, cuda, c):
    """pack_relu_mlp(x3=True) on selection weights (+-2^e: no mid piece) = the same network packed with x3=False and fed
    r16(inputs) = bf16(x) + bf16(x - bf16(x)), bit for bit: r16 is idempotent, so only the first layer's inputs lose bits.  With
    init tables the input block never passes a split stage: both packs are then fed r16(inputs)."""
    hip, fused = mods
    net = lc.build_x3_net(c)
    Ws, bs = [w.to(cuda) for w in net.Ws], [b.to(cuda) for b in net.bs]
    pkx = fused.pack_relu_mlp(Ws, bs, net.din_a, net.din_b, net.skip_at, precompute=c['precompute'], x3=True)
    pk0 = fused.pack_relu_mlp(Ws, bs, net.din_a, net.din_b, net.skip_at, precompute=c['precompute'], x3=False)
    assert pkx.desc.w_format == hip.W_BF16X2 and pk0.desc.w_format == hip.W_F32
    ta, tb = net.tab_a.to(cuda), net.tab_b.to(cuda)
    ra, rb = lc.r16(net.tab_a).to(cuda), lc.r16(net.tab_b).to(cuda)
    assert not torch.equal(ra, ta)
    orders = ('row', 'point') if c['form'] == 'orders' else (None,)
    for order in orders:
        want = _run_c1(c, net, pk0, ra, rb, mods, cuda, order)
        got = _run_c1(c, net, pkx, ra if c['precompute'] else ta, rb if c['precompute'] else tb, mods, cuda, order)
        assert torch.equal(got, want), '%s order=%s: %s' % (c['id'], order, _diff(got, want))
        if c['live'] is not None:
            dead = torch.from_numpy(mc.dead_rows(c, c['live'])).to(cuda)
            assert int(dead.sum()) == 64 and bool((got[dead].view(torch.int32) == 0).all())
            plain = _run_c1(dict(c, live=None), net, pkx, ra, rb, mods, cuda, order)
            assert torch.equal(got[~dead], plain[~dead])
        else:   # ... and it is the float64 statement of the network on r16(inputs)
            cr = dict(c)
            netr = lc.build_x3_net(cr)
            netr.tab_a, netr.tab_b = lc.r16(net.tab_a), lc.r16(net.tab_b)
            ref = lc.x3_reference(netr, check=False)['out']
            if not c['precompute']:   # (U + V of a single-column row is one product: no rounded addition to mirror)
                assert torch.equal(got.cpu(), ref.float()), _diff(got.cpu(), ref.float())


def test_bf16x2_stages_random_weights_vs_modelled_arithmetic(mods, cuda):
    """C2: one softplus geometry chain (pack_geo_chains(x3=True)['fwd']: logit, feature head and every dumped layer) and one
    occupancy launch with the in-kernel encoding, random weights, against the float64 evaluation of the MODELLED arithmetic
    (lowp_cases.x3dot: operands bf16(x) + bf16(x - bf16(x)), products hi hi + hi mid + mid hi); reference arithmetic = the same
    model in float32 on the CPU."""
    hip, fused = mods
    Q, skip = 129, 2
    Ws, bs = lc.geo_weights(7)
    pts = (torch.rand(Q, 3, generator=torch.Generator().manual_seed(3)) * 2 - 1)
    pe = hip.pe_encode(pts.to(cuda), lc.OCC_OCTAVES, out_stride=64, scale=lc.OCC_SCALE)
    chains = fused.pack_geo_chains([w.to(cuda) for w in Ws], [b.to(cuda) for b in bs], [skip], lc.OCC_DPE, x3=True)
    pk = chains['fwd']
    assert pk.desc.w_format == hip.W_BF16X2
    dumps = [nan_buffer(Q, 256, cuda) for _ in range(len(Ws))]
    whole, out = nan_buffer(Q, 1, cuda)
    path = hip.PsnMlpPath()
    pk(pe, Q, save=[d for _, d in dumps], out=out, path=path)
    assert guards_intact(whole, Q) and all(guards_intact(w_, Q) for w_, _ in dumps)
    assert path.chain == 1 and path.x3 == 1 and path.width16 == 16
    t64, t32 = lc.geo_chain_model(Ws, bs, skip, pe.cpu(), torch.float64), lc.geo_chain_model(Ws, bs, skip, pe.cpu(), torch.float32)
    record('bf16x2/chain', 'C2-chain logit', out, t64[0], t32[0])
    record('bf16x2/chain', 'C2-chain features', dumps[-1][1], t64[1], t32[1])
    for l in range(len(Ws) - 1):
        o = Ws[l].shape[0]
        record('bf16x2/chain', 'C2-chain dump%d' % l, dumps[l][1][:, :o], t64[2][l], t32[2][l])
    # the exact chain on the same inputs differs: the split stages really ran
    pk0 = fused.pack_geo_chains([w.to(cuda) for w in Ws], [b.to(cuda) for b in bs], [skip], lc.OCC_DPE, x3=False)['fwd']
    assert not torch.equal(pk0(pe, Q, save=[torch.empty(Q, 256, device=cuda) for _ in range(len(Ws))]), out)
    # occupancy launch, encoding formed in the kernel: raw weights, 1 / sqrt 2 folded in by the packer
    inv = 1.0 / 2.0 ** 0.5
    Wr = [w.clone() for w in Ws]
    Wr[skip] = Ws[skip] * 1.4
    We = [w if l != skip else w * inv for l, w in enumerate(Wr)]      # the packer's fold, in its float32 arithmetic
    pko = fused.pack_geo_occupancy([w.to(cuda) for w in Wr], [b.to(cuda) for b in bs], [skip], lc.OCC_DPE, x3=True)
    whole, occ = nan_buffer(Q, 1, cuda)
    pko.on_points(pts.to(cuda), lc.OCC_OCTAVES, lc.OCC_SCALE, out=occ)
    assert guards_intact(whole, Q)
    xs32 = pts * torch.tensor(lc.OCC_SCALE, dtype=torch.float32)
    res = []
    for dt in (torch.float64, torch.float32):
        logit = lc.geo_chain_model(We, bs, skip, mc.pe_columns(xs32, lc.OCC_OCTAVES, dt), dt)[0]
        res.append(torch.sigmoid(logit * -10.0))
    record('bf16x2/occupancy', 'C2-occupancy', occ, res[0], res[1])
