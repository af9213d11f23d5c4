"""The stage-2 train step on the GPU -- TrainStep._fwd_bwd: which rows ride in which launch, which cotangents are added where,
LightRows / ScatterRows / normalize_rows, the side stream, the device-side mask count, the hand-over of the gradients -- against
the float64 value of the reference's step, EVERY parameter gradient and both light tables, under the gate of
tests/step_grad_cases.py (allowance = 8 x the reference arithmetic's own distance from float64, tensor form and row form).
One case per path the step can take (step_grad_cases.CASES); each asserts from ops.HITS that it ran on the engines it is meant
to exercise."""
import pytest
import torch

from tests import step_grad_cases as sg

pytestmark = pytest.mark.gpu

# forward counts of the autograd nodes (ops.HITS) by path; a node that is not listed must not have run at all
ENGINES = ('VisibilityPair', 'FusedPairMLP', 'ReluMLP', 'FusedReluNet', 'SGShade', 'MFShade', 'ScatterRows', 'Stage2Losses', 'LightRows')
PAIR = dict(VisibilityPair=1, FusedReluNet=3, SGShade=1, ScatterRows=1, Stage2Losses=1, LightRows=1)  # the benchmark's path
HITS = {
    'microfacet': dict(PAIR, SGShade=0, MFShade=1),
    'no_surface': dict(Stage2Losses=1, LightRows=1),  # nothing but the table rows and the (constant) losses is launched
    # the batch's lights as given: no table lookup; the L shading rows carry the visibility loss's gradient through the
    # gradient-capable pair engine, whose backward re-evaluates the rows layer by layer (one ReluMLP)
    'given_lights': dict(PAIR, VisibilityPair=0, LightRows=0, FusedPairMLP=1, ReluMLP=1),
    # no fused pair launch once a gradient may reach the shading rows or the light directions: the supervised rows take the
    # layer-wise formulation on the expanded [V Ns, 128] input (one ReluMLP), the shading rows the gradient-capable pair engine,
    # whose backward re-evaluates them layer by layer (the second ReluMLP; with the colour detached its cotangent is all zero)
    'light_vis_attached': dict(PAIR, VisibilityPair=0, FusedPairMLP=1, ReluMLP=2),
    'vis_rgb_attached': dict(PAIR, VisibilityPair=0, FusedPairMLP=1, ReluMLP=2),
    'vis_both_attached': dict(PAIR, VisibilityPair=0, FusedPairMLP=1, ReluMLP=2),
}


def _step(cuda, ci, extra=None):
    """s2.PSNetwork + s2.TrainStep on the device from the case's state dict and table, in the phase's train_fix state."""
    import psnerf_amd.stage2 as s2
    conf = s2.bear_conf(**dict(ci['conf_overrides'], **{'loss.loss_type': ci['loss_type']}, **(extra or {})))
    net = s2.PSNetwork(conf)
    net.load_state_dict(ci['sd'])
    net.to(cuda)
    step = s2.TrainStep(net, conf, ci['light_init'].shape[0], ci['light_init'].to(cuda), cuda)
    step.train_fix()  # iteration 0
    step.cur_iter = 1
    if ci['phase'] == 2:
        step.cur_iter = 5000
        step.train_fix()
        step.cur_iter = 5001
    return step


def _grads(step):
    gr = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in step.model.named_parameters()}
    for k, t in (('__light_dir', step.light_para.weight), ('__light_int', step.light_inten_para.weight)):
        gr[k] = None if t.grad is None else t.grad.detach().clone()
    return gr


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _run(cuda, name, edit=None, extra=None, count=None, batch=None, noise=None):
    """One _fwd_bwd of the case on the device -> (gradients, ops.HITS of the call)."""
    from psnerf_amd import ops
    ci, _, _ = sg.case_data(name)
    step = _step(cuda, ci, extra)
    inp, gt = batch if batch is not None else ci['batch']
    inp, gt = _to(inp, cuda), _to(gt, cuda)
    nz = _to(noise if noise is not None else ci['noise'], cuda)
    if edit is not None:
        edit(inp, nz)
    ops.HITS.clear()
    step._fwd_bwd(inp, gt, ci['l_slt'].to(cuda), noise=nz, count=count)
    torch.cuda.synchronize()
    hits = dict(ops.HITS)
    print('step-grad %-18s engines %s' % (name, ' '.join('%s=%d' % (k, hits[k]) for k in ENGINES if hits.get(k))))
    return _grads(step), hits


def _assert_engines(name, hits, times=1):
    want = HITS.get(name, PAIR)
    got = {k: hits.get(k, 0) for k in ENGINES}
    assert got == {k: times * want.get(k, 0) for k in ENGINES}, (name, got)


def _with_surface_idx(inp, nz):
    inp['surface_idx'] = inp['surface_mask'][0].nonzero(as_tuple=True)[0]


def _padded(capacity, with_count):
    def edit(inp, nz):
        from psnerf_amd import hip
        ns = int(inp['surface_mask'].sum())
        assert capacity > ns
        inp['surface_idx'], cnt = hip.surface_index(inp['surface_mask'][0].contiguous(), capacity)
        if with_count:
            inp['surface_count'] = cnt
        for k in list(nz):  # the jitter draw of a padded list has one row per slot; the dead rows' draws are never used
            full = torch.zeros(capacity, 3, device=nz[k].device)
            full[:ns] = nz[k]
            nz[k] = full
    return edit


EDITS = {
    'surface_idx': _with_surface_idx,
    'padded_count': _padded(576, True),   # 9 blocks of 64 rows: the visibility launch skips the padding's shading rows (live count)
    'padded': _padded(602, False),        # padded to the pixel count, no count: every slot is evaluated, the dead rows add nothing
}
PLAIN = [k for k in sg.CASES if k not in ('no_overlap', 'global_count')]


@pytest.mark.parametrize('name', PLAIN)
def test_step_gradients_vs_float64(cuda, name):
    _, ref, truth = sg.case_data(name)
    grads, hits = _run(cuda, name, edit=EDITS.get(name))
    _assert_engines(name, hits)
    sg.check(grads, ref, truth, name)
    if name == 'no_surface':
        assert all(g is None or not bool(g.any()) for g in grads.values())


def test_side_stream_off_gives_the_same_bits(cuda):
    """train.overlap_small_nets off: the BRDF / normal nets queue behind the visibility launch instead of beside it.  One
    _fwd_bwd, every gradient bit for bit the default case's (and inside the gate)."""
    _, ref, truth = sg.case_data('default')
    g1, h1 = _run(cuda, 'default')
    g0, h0 = _run(cuda, 'no_overlap', extra=sg.CASES['no_overlap']['over'])
    _assert_engines('no_overlap', h0)
    assert h0 == h1
    sg.check(g0, ref, truth, 'no_overlap')
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None) and (g0[k] is None or torch.equal(g0[k], g1[k])), k


def test_pixel_shards_with_the_global_count_sum_to_the_full_batch(cuda):
    """What pixel data parallelism relies on: two pixel shards, each through _fwd_bwd with the FULL batch's masked-pixel count
    as a device tensor; their summed gradients against the float64 truth of the full batch, under the same gate."""
    ci, ref, truth = sg.case_data('default')
    inp, gt = ci['batch']
    n = inp['uv'].shape[1]
    surf = inp['surface_mask'][0]
    rank = torch.cumsum(surf.long(), 0) - 1
    count = (inp['surface_mask'] & inp['object_mask']).sum().float().reshape(1).to(cuda)
    total, hits = {}, {}
    for idx in (torch.arange(0, n // 2), torch.arange(n // 2, n)):
        noise = {k: v[rank[idx][surf[idx]]] for k, v in ci['noise'].items()}
        g, h = _run(cuda, 'global_count', count=count, batch=sg.sub_batch(inp, gt, idx), noise=noise)
        for k, v in g.items():
            if v is not None:
                total[k] = total.get(k, 0) + v.double().cpu()
        for k, v in h.items():
            hits[k] = hits.get(k, 0) + v
    _assert_engines('global_count', hits, times=2)
    sg.check(total, ref, truth, 'global_count')
