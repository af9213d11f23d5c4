"""The stage-1 train step on the GPU -- the double backward through the geometry chains with the normal points riding behind the
render rows (feat_rows / SplitRows), the appearance chains, the composite backward, SurfaceNormals, Stage1Losses and the weight
normalisation underneath -- against the float64 value of the reference's step, EVERY parameter gradient, under the gate of
tests/step_grad_cases.py (allowance = 8 x the reference arithmetic's own distance from float64, tensor form and row form).  One
case per path the step can take (tests/step1_grad_cases.py CASES); each asserts from ops.HITS which engines ran, and that no other
did.

The surface is an input of the step: ``_seam`` wraps the renderer's ``_surface``, lets the product's own sweep / prefetch hand-over
/ psn_surface_points run, asserts that its mask is the case's and its depths within helpers.ATOL_DEPTH of the case's, and hands on
the case's depths and mask with the points formed from them in fp32 on the device."""
import pytest
import torch

from psnerf_amd.synthetic import stage1_cfg
from tests import step1_grad_cases as s1
from tests.helpers import ATOL_DEPTH, assert_close

pytestmark = pytest.mark.gpu

# forward counts of the autograd nodes (ops.HITS) by path; a node that is not listed must not have run at all.
#   WeightNormAll: one launch per set of effective matrices -- the occupancy pack of the march (built once, cached), then
#   _geo_params and _app_params per call that needs them: render_and_gradient asks for the geometry set once before it decides on
#   its one-launch form (+ the appearance set: 3 in all); forward() + gradient() ask 2 + 1 (reference-shaped: 4; behind a
#   render_and_gradient that fell apart: 5); the layer-wise appearance net asks twice (_app_parts, then _app: 6).
#   chunked: MAX_ROWS = 1000 < 8,580 rows, so render_and_gradient falls apart into forward() -- 8,320 render rows = 8 x 1000 + 320
#   = nine GeoFieldFused calls whose parameter gradients autograd accumulates -- and gradient() on the 260 normal rows: ten.
ENGINES = ('GeoFieldFused', 'AppNetFused', 'GeoField', 'ReluMLP', 'SplitRows', 'AlphaComposite', 'SurfaceNormals', 'Stage1Losses',
           'WeightNormAll')
FUSED = dict(GeoFieldFused=1, AppNetFused=1, SplitRows=2, AlphaComposite=1, SurfaceNormals=1, Stage1Losses=1, WeightNormAll=3)
LAYERWISE = dict(GeoField=2, ReluMLP=1, AlphaComposite=1, SurfaceNormals=1, Stage1Losses=1, WeightNormAll=6)
HITS = {
    'reference_shaped': dict(GeoFieldFused=2, AppNetFused=1, AlphaComposite=1, WeightNormAll=4),
    'torch_glue': dict(FUSED, SurfaceNormals=0, Stage1Losses=0),
    'layerwise': LAYERWISE,
    'h64': LAYERWISE,
    'chunked': dict(FUSED, GeoFieldFused=10, SplitRows=0, WeightNormAll=5),
    # prefetch_surface packs the chains while the sweep runs (+ 2), the step re-packs the occupancy network behind the update (+ 1)
    'trainer': dict(FUSED, WeightNormAll=6),
}


def _to(v, dev):
    if isinstance(v, dict):
        return {k: _to(x, dev) for k, x in v.items()}
    return v.to(dev) if torch.is_tensor(v) else v


def _seam(ren, dists, mask, calls):
    """See the module docstring."""
    inner = ren._surface

    def surface(pixels, camera_mat, world_mat, ray_steps):
        cam, rays, d, m, _ = inner(pixels, camera_mat, world_mat, ray_steps)
        want_d, want_m = dists.to(d.device), mask.to(d.device)
        assert torch.equal(m.bool(), want_m), 'the product\'s hit mask is not the case\'s'
        if bool(want_m.any()):
            assert float((d - want_d)[want_m].abs().max()) <= ATOL_DEPTH
        calls.append(1)
        return cam, rays, want_d, want_m, (cam + rays * want_d.unsqueeze(-1)).view(-1, 3)
    ren._surface = surface


def _net(cuda, ci, name, cfg=None):
    from psnerf_amd.stage1 import NeuralNetwork, Renderer
    cfg = cfg or stage1_cfg('bunny', **ci['over'])
    net = NeuralNetwork(cfg)
    net.load_state_dict(ci['sd'])
    ren = Renderer(net, cfg, device=cuda)
    ren.sync_free = name != 'reference_shaped'
    if name == 'torch_glue':
        ren.FUSED_GLUE = False
    if name == 'layerwise':
        net.USE_FUSED_CHAINS = False
    if name == 'chunked':
        net.MAX_ROWS = 1000
    return cfg, net, ren


def _engines(name, hits, times=1):
    print('%s %-18s engines %s' % (s1.PREFIX, name, ' '.join('%s=%d' % (k, hits[k]) for k in ENGINES if hits.get(k))))
    want = HITS.get(name, FUSED)
    got = {k: hits.get(k, 0) for k in ENGINES}
    assert got == {k: times * want.get(k, 0) for k in ENGINES}, (name, got)


def _run(cuda, name, rays=None, loss_edit=None):
    """One forward + loss + backward of the case (of its rays ``rays``) on the device -> (gradients, ops.HITS of the call)."""
    from psnerf_amd import ops
    from psnerf_amd.stage1 import Loss
    ci, _, _ = s1.case_data(name)
    n = ci['mask'].shape[0]
    idx = torch.arange(n) if rays is None else rays
    cfg, net, ren = _net(cuda, ci, name)
    calls = []
    _seam(ren, ci['dists'][idx], ci['mask'][idx], calls)
    sub = lambda t: None if t is None else t[:, idx].contiguous().to(cuda)
    noise = {k: v[idx].contiguous().to(cuda) for k, v in ci['noise'].items()}
    ops.HITS.clear()
    out = ren(sub(ci['pix']), ci['K'].to(cuda), ci['c2w'].to(cuda), ci['S'].to(cuda), 'unisurf', add_noise=True, eval_=False,
              it=ci['it'], noise=noise)
    assert calls == [1] and (out.get('diff_norm_full') is not None) == ren.sync_free
    loss = Loss(*ci['weights'], device=cuda)
    if name == 'torch_glue':
        loss.fused = False
    if loss_edit is not None:
        loss_edit(loss)
    terms = loss(out, sub(ci['rgb_gt']), sub(ci['normal_gt']), sub(ci['norm_mask']), out['acc_map'] if ci['mask_gt'] is not None else None,
                 sub(ci['mask_gt']), sub(ci['mask_valid']))
    terms['loss'].backward()
    torch.cuda.synchronize()
    hits = dict(ops.HITS)
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}, hits


PLAIN = [k for k in s1.CASES if k not in ('ray_shards', 'trainer')]


@pytest.mark.parametrize('name', PLAIN)
def test_step1_gradients_vs_float64(cuda, name):
    _, ref, truth = s1.case_data(name)
    grads, hits = _run(cuda, name)
    _engines(name, hits)
    s1.check(grads, ref, truth, name, s1.PREFIX)


@pytest.mark.parametrize('name', ['reference_shaped', 'torch_glue', 'chunked'])
def test_other_formulations_of_the_default_step_agree_with_it(cuda, name):
    """The reference-shaped path, the torch glue and the chunked geometry calls against the default case's DEVICE gradients under
    the max-normalised 1e-4 of test_sync_free_training_forward_matches_reference_shaped_path.  None of the three promises equal
    bits: the reference-shaped path evaluates the normals on the compacted hit points in a launch of their own, the torch glue
    replaces kernels by torch formulas, and the chunked form sums every geometry parameter's gradient over ten launches."""
    g0, _ = _run(cuda, 'default')
    g1, _ = _run(cuda, name)
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert_close(g1[k].cpu(), g0[k].cpu(), 1e-4, '%s grad %s' % (name, k))


def test_ray_shards_with_the_global_counts_sum_to_the_full_batch(cuda):
    """What ray data parallelism relies on: the two halves of the default case's rays, each through forward + Loss with the FULL
    batch's ray count (Loss.global_rays) and its three device-side counts (Loss.global_counts) set by hand; their gradients,
    summed in float64, against the float64 truth of the full batch under the same gate.  No process group is involved."""
    ci, ref, truth = s1.case_data('ray_shards')
    n = ci['mask'].shape[0]
    counts = torch.tensor([float(ci['mask'].sum()), float(ci['norm_mask'].sum()), float(n)], device=cuda)

    def edit(loss):
        loss.global_rays = lambda: n
        loss.global_counts = lambda t: t.copy_(counts)
    total, hits = {}, {}
    for idx in (torch.arange(0, n // 2), torch.arange(n // 2, n)):
        g, h = _run(cuda, 'ray_shards', rays=idx, loss_edit=edit)
        for k, v in g.items():
            if v is not None:
                total[k] = total.get(k, 0) + v.double().cpu()
        for k, v in h.items():
            hits[k] = hits.get(k, 0) + v
    _engines('ray_shards', hits, times=2)
    s1.check(total, ref, truth, 'ray_shards', s1.PREFIX)


def _train_step(cuda, flat):
    """Trainer.train_step on the ``trainer`` case -> (the gradients the optimiser received, ops.HITS)."""
    from psnerf_amd import ops
    from psnerf_amd.optim import FlatAdam
    from psnerf_amd.stage1 import Trainer
    ci, _, _ = s1.case_data('trainer')
    cfg, net, ren = _net(cuda, ci, 'trainer', stage1_cfg('bunny', **s1.trainer_cfg_overrides(ci)))
    opt = (FlatAdam if flat else torch.optim.Adam)(net.parameters(), lr=1e-4)
    tr = Trainer(ren, opt, cfg, device=cuda)
    calls, got = [], {}
    _seam(ren, ci['dists'], ci['mask'], calls)
    names = {p: k for k, p in net.named_parameters()}
    inner = opt.step

    def step(*a, **kw):
        got['handed'] = {names[p]: p.grad.detach().clone() for p in names if p.grad is not None}
        r = inner(*a, **kw)
        if flat:  # what the flat bucket received: the slot views the gathered gradients were copied into
            got['bucket'] = {names[p]: opt._flat['gview'][p].detach().clone() for p in names if p in opt._flat['gview']}
        return r
    opt.step = step
    ops.HITS.clear()
    terms = tr.train_step(ci['data'], it=ci['it'], pix=ci['pix'].clone(), noise=_to(ci['noise'], cuda))
    torch.cuda.synchronize()
    assert calls == [1] and 'normal_loss' in terms and 'mask_loss' not in terms
    if flat:
        assert sorted(got['bucket']) == sorted(got['handed']) and all(torch.equal(got['bucket'][k], got['handed'][k]) for k in got['handed'])
    return got['bucket' if flat else 'handed'], dict(ops.HITS)


def test_trainer_step_hands_the_optimiser_the_gated_gradients(cuda):
    """The step through Trainer.train_step (stage1_targets, the pinned upload, prefetch_surface, attach_grads, the weight-pack
    invalidation) on a stage1_batch data dict with injected pixels and per-ray draws, once with torch.optim.Adam and once with
    optim.FlatAdam: what each optimiser received before its update goes through the gate (the truth uses the same targets, gathered
    by o1.gather_pixels), and both received equal bits."""
    _, ref, truth = s1.case_data('trainer')
    res = []
    for flat in (False, True):
        grads, hits = _train_step(cuda, flat)
        _engines('trainer', hits)
        s1.check(grads, ref, truth, 'trainer/' + ('FlatAdam' if flat else 'Adam'), s1.PREFIX)
        res.append(grads)
    assert sorted(res[0]) == sorted(res[1])
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
