"""The stage-1 train step's gradients, parameter by parameter, against float64: restated step, truth, reference and cases (no GPU).

``step_gradients`` runs ONE stage-1 step in ONE dtype: o1.Renderer.unisurf (training forward, stratified jitter on) -> o1.Loss ->
backward.  At float32 it IS the reference arithmetic (tests/test_step1_grad_cpu.py anchors it to o1.Trainer.compute_loss +
backward); at float64, with the fp32 weights, pixels, camera, targets, jitter tables and surface cast up, it is the exact value of
the reference formulas for those inputs (the truth).  The gate is the stage-2 one, imported: tests/step_grad_cases.py (figures,
measure, report_line, check, FACTOR, ROW_FLOOR, MARGIN).

THE SURFACE IS AN INPUT OF THE STEP.  d_i and the hit mask come out of a gradient-free march and enter the differentiable part
detached; the march and the root finder have bit-level tests of their own.  A case carries ``dists [N]`` and ``mask [N]``, computed
once by the fp32 oracle's ``_surface``; all three evaluations (truth, reference, product) start from them (``_SeamRenderer`` here,
the wrapper of tests/test_step1_grad_gpu.py on the device).

Cases are built from seeds, and the builder asserts what it promises:
 (a) rays come from a seeded pool of pixels of a 48 x 64 synthetic view; a ray is eligible only if the fp32 oracle and its float64
     evaluation, each marching on its own, agree about hit / miss (keeps the seam's mask assertion away from the silhouette);
 (b) targets are synthetic per-ray tensors (the ``trainer`` case: planes of a stage1_batch); every rgb - rgb_gt and every masked
     normal - normal_gt keeps MARGIN from 0 in float64 (the kink of an L1 term), and a ray whose acc lies within MARGIN of 0 or 1 is
     left out of mask_valid (the BCE's clamp and -100 log floor);
 (c) the jitter draw of every (ray, sample) row is the first of K = 8 candidates for which every one of the appearance net's
     4 x 256 ReLU pre-activations of that row keeps MARGIN from 0 in float64 (the geometry net is smooth); a ray that holds a row
     without a clear candidate is replaced by the next eligible ray;
 (d) loss weights: besides one case at the shipped weights (1.0, 0.005, 0.05, 1.0) the cases use WEIGHTS = (1.0, 0.5, 0.5, 1.0),
     at which every enabled term contributes at least 10 % of max|gradient| on at least one geometry tensor in float64
     (tests/test_step1_grad_cpu.py measures and prints the shares; at the shipped weights the smoothness term is below 1 %).

MARGIN = 2e-5 (step_grad_cases.MARGIN): four times the largest difference between an fp32 and a float64 appearance pre-activation
(4.9e-6 on the default case's 8,320 rows x 1,024 units; tests/test_step1_grad_cpu.py re-measures and prints it).  About 86 % of the
rows are clear at the first draw; of 142 candidate rays of the default case 9 held a row without a clear draw among 8.

Measured (CPU, 8 threads; tests/test_step1_grad_cpu.py prints them): the reference sits E_t = 9e-7 (shipped weights) to 9e-6
(WEIGHTS: the smoothness and normal terms, second derivatives of the geometry net, are the noisier ones) from float64 on the
default case, E_r = 7e-5 to 1e-4; the float64 march finds the same masks on all 420 pool pixels and depths within 1.6e-6.
"""
import torch

from oracle import stage1 as o1
from psnerf_amd.synthetic import stage1_batch, stage1_camera, stage1_cfg
from tests.helpers import stage1_state_dict
from tests.step_grad_cases import FACTOR, MARGIN, ROW_FLOOR, check, figures, measure, report_line  # noqa: F401  (the gate, re-exported)

H, W = 48, 64                        # the synthetic view
POOL, POOL_SEED = 420, 77            # pixels classified once per network (fp32 and float64 march)
K_DRAWS = 8                          # candidate jitter tables per case
SPARE = 12                           # rays beyond N whose rows are examined, to replace rays without a clear draw
SHIPPED = (1.0, 0.005, 0.05, 1.0)    # lambda_l1_rgb, lambda_normals, lambda_normloss, lambda_mask of the configurations
WEIGHTS = (1.0, 0.5, 0.5, 1.0)       # (d): no term hides
MUTANTS = ('smooth_w', 'normal_w', 'mask_w', 'nbr_detached', 'drop_ray', 'drop_sample', 'feat_row', 'last_feat_row',
           'hit_count_plus_one', 'rays_local')
PREFIX = 'step1-grad'                # of the report lines


def _up(v, dtype):
    if isinstance(v, dict):
        return {k: _up(x, dtype) for k, x in v.items()}
    if torch.is_tensor(v):
        v = v.detach().cpu()
        return v.to(dtype) if v.dtype == torch.float32 else v
    return v


def group_noise(noise, hit):
    """Per-ray tables {'full' [N, S], 'nbr_full' [N, 3]} -> the group-sized tables of the reference's draw order."""
    return {'miss': noise['full'][~hit].unsqueeze(0), 'hit': noise['full'][hit].unsqueeze(0), 'nbr': noise['nbr_full'][hit]}


# ------------------------------------------------------------------------------------------------ the restated step
class _SeamRenderer(o1.Renderer):
    """o1.Renderer whose ``_surface`` takes depths and mask from the case: cam and rays in the evaluation dtype,
    points = cam + rays * dists."""
    seam = None  # (dists [N] fp32, mask [N])

    def _surface(self, pixels, camera_mat, world_mat, ray_steps):
        n = pixels.shape[1]
        cam = o1.camera_origin(n, world_mat)
        rays = o1.pixel_rays(pixels, camera_mat, world_mat)
        rays = rays / rays.norm(2, 2).unsqueeze(-1)
        cam, rays = cam.reshape(-1, 3), rays.reshape(-1, 3)
        dists = self.seam[0].to(rays.dtype)
        points = (cam + rays * dists.unsqueeze(-1)).view(-1, 3)
        return cam, rays, dists, self.seam[1], points


class _Net(o1.NeuralNetwork):
    """o1.NeuralNetwork with the in-network mutants (None: the oracle's network unchanged)."""
    mutant = None
    n_hit = 0      # hit rays of the batch
    first_hit = 0  # index of the first hit ray
    n_samples = 0

    def gradient(self, p, tflag=True):
        g = super().gradient(p, tflag)
        if self.mutant == 'nbr_detached' and p.shape[0] == 2 * self.n_hit:  # the surface-normal call: [surface | neighbours]
            g = torch.cat([g[:self.n_hit], g[self.n_hit:].detach()], 0)
        return g

    def _first_occupied(self, alpha):
        s = self.n_samples
        ray = alpha.reshape(-1)[self.first_hit * s:(self.first_hit + 1) * s]
        return self.first_hit * s + int((ray > 0.5).nonzero()[0])  # the first occupied sample of the first hit ray

    def infer_app(self, points, normals, view_pe, feat):
        if self.mutant == 'last_feat_row':
            feat = torch.cat([feat[:-1], feat[-1:].detach()], 0)
        if self.mutant == 'feat_row':  # the same on a row that carries composite weight
            with torch.no_grad():
                j = self._first_occupied(torch.sigmoid(self.infer_occ(points)[..., :1] * -10.0))
            feat = torch.cat([feat[:j], feat[j:j + 1].detach(), feat[j + 1:]], 0)
        return super().infer_app(points, normals, view_pe, feat)

    def forward(self, p, ray_d=None, **kw):
        r = super().forward(p, ray_d, **kw)
        if self.mutant == 'drop_sample' and kw.get('return_addocc'):
            rgb, a = r
            j = self._first_occupied(a.detach())
            one = torch.zeros(a.shape[0], 1, dtype=torch.bool)
            one[j] = True
            r = torch.where(one, rgb.detach(), rgb), torch.where(one, a.detach(), a)
        return r


def step_gradients(dtype, cfg_overrides, state_dict, case, mutant=None, seam=True, weights=None, probe=None, forward_only=False):
    """{name: float64 tensor} of every parameter's gradient of ONE stage-1 step evaluated in ``dtype`` (zeros for a parameter the
    loss does not reach).  ``mutant``: one deliberate error (MUTANTS), used only to show that the gate can fail.  seam=False: the
    oracle's own march instead of the case's surface (the anchor test).  weights: other loss weights than the case's (the term
    shares).  probe: a dict that receives 'pre_min' [N S], the smallest |appearance pre-activation| per sample row, the forward
    outputs 'rgb', 'normal_pred', 'acc_map' (detached) and, if it holds 'pre' = [], the pre-activations themselves; forward_only:
    return None after the forward (the case builder)."""
    assert mutant is None or mutant in MUTANTS, mutant
    cfg = stage1_cfg('bunny', **cfg_overrides)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)  # the oracle allocates its tables and dense outputs with the default dtype
    try:
        hit = case['mask']
        n = hit.shape[0]
        net = _Net(cfg)
        net.load_state_dict(state_dict)
        net = net.to(dtype)
        net.mutant, net.n_hit, net.n_samples = mutant, int(hit.sum()), case['noise']['full'].shape[1]
        net.first_hit = int(hit.nonzero()[0]) if net.n_hit else 0
        ren = _SeamRenderer(net, cfg) if seam else o1.Renderer(net, cfg)
        ren.seam = (case['dists'], hit)
        c = _up({k: v for k, v in case.items() if torch.is_tensor(v) or isinstance(v, dict)}, dtype)
        hooks = []
        if probe is not None:
            probe['pre_min'] = torch.full((n * net.n_samples,), float('inf'), dtype=torch.float64)

            def seen(mod, i, o):
                probe['pre_min'] = torch.minimum(probe['pre_min'], o.detach().abs().min(-1).values.double())
                if 'pre' in probe:
                    probe['pre'].append(o.detach().double())
            hooks = [getattr(net, 'lina%d' % l).register_forward_hook(seen) for l in range(net.n_app - 1)]
        out = ren(c['pix'], c['K'], c['c2w'], c['S'], 'unisurf', add_noise=True, eval_=False, it=case['it'],
                  noise=group_noise(c['noise'], hit))
        for h in hooks:
            h.remove()
        assert torch.equal(out['mask_pred'], hit)
        if probe is not None:
            probe.update({k: out[k].detach().double() for k in ('rgb', 'normal_pred', 'acc_map')})
        if forward_only:
            return None
        w = list(case['weights'] if weights is None else weights)
        for key, i in (('smooth_w', 1), ('normal_w', 2), ('mask_w', 3)):
            if mutant == key:
                w[i] = w[i] * 0.99
        if mutant == 'rays_local':  # the rgb term divided by a shard's ray count instead of the batch's
            w[0] = w[0] * n / (n // 2)
        if mutant == 'hit_count_plus_one':
            out['diff_norm'] = out['diff_norm'] * (net.n_hit / (net.n_hit + 1.0))
        if mutant == 'drop_ray':  # the first hit ray contributes nothing to the backward pass
            one = torch.zeros(n, dtype=torch.bool)
            one[net.first_hit] = True
            out['rgb'] = torch.where(one[None, :, None], out['rgb'].detach(), out['rgb'])
            out['normal_pred'] = torch.where(one[None, :, None], out['normal_pred'].detach(), out['normal_pred'])
            out['acc_map'] = torch.where(one[None], out['acc_map'].detach(), out['acc_map'])
            out['diff_norm'] = torch.cat([out['diff_norm'][:1].detach(), out['diff_norm'][1:]])
        terms = o1.Loss(*w)(out, c['rgb_gt'], c.get('normal_gt'), case.get('norm_mask'), out['acc_map'], c.get('mask_gt'),
                            case.get('mask_valid'))
        if terms['loss'].requires_grad:  # (no graph: every enabled term is a constant, e.g. smoothness + normal term without a hit ray)
            terms['loss'].backward()
        return {k: (p.grad.detach().double() if p.grad is not None else torch.zeros(p.shape, dtype=torch.float64))
                for k, p in net.named_parameters()}
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------ (a) the pool
_POOLS = {}


def _march(dtype, cfg, sd, pix, K, c2w):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        net = o1.NeuralNetwork(cfg)
        net.load_state_dict(sd)
        ren = o1.Renderer(net.to(dtype), cfg)
        with torch.no_grad():
            _, _, dists, mask, _ = ren._surface(_up(pix, dtype), _up(K, dtype), _up(c2w, dtype), cfg['rendering']['ray_marching_steps'])
        return dists.detach(), mask
    finally:
        torch.set_default_dtype(old)


def pool(cfg_overrides, sd_seed):
    """dict(pix [P, 2], dists [P] fp32, mask [P], eligible [P], depth_diff) of the seeded pixel pool for one network: classified
    once by the fp32 oracle and once by its float64 evaluation, each marching on its own.  Cached per process."""
    model_over = {k: v for k, v in cfg_overrides.items() if k.startswith('model.')}
    key = (tuple(sorted(model_over.items())), sd_seed)
    if key not in _POOLS:
        cfg = stage1_cfg('bunny', **model_over)
        sd = stage1_state_dict(cfg, seed=sd_seed)
        K, c2w, _ = stage1_camera(cfg, h=H, w=W)
        idx = torch.randperm(H * W, generator=torch.Generator().manual_seed(POOL_SEED))[:POOL]
        pix = torch.stack([(idx % W).float(), (idx // W).float()], -1)[None]
        d32, m32 = _march(torch.float32, cfg, sd, pix, K, c2w)
        d64, m64 = _march(torch.float64, cfg, sd, pix, K, c2w)
        both = m32 & m64
        _POOLS[key] = dict(pix=pix[0], dists=d32, mask=m32, eligible=m32 == m64,
                           depth_diff=float((d32.double() - d64)[both].abs().max()) if bool(both.any()) else 0.0)
    return _POOLS[key]


# ------------------------------------------------------------------------------------------------ (c) clear jitter draws
class _Recorder(torch.nn.Module):
    """Stands in for the network while the oracle forms its sample points: records them, evaluates nothing."""

    def __init__(self):
        super().__init__()
        self.p = None

    def forward(self, p, ray_d=None, **kw):
        self.p, self.view = p.detach(), ray_d.detach()
        return torch.zeros(p.shape[0], 3, dtype=p.dtype), torch.zeros(p.shape[0], 1, dtype=p.dtype)

    def gradient(self, p, tflag=True):
        return torch.ones(p.shape[0], 1, 3, dtype=p.dtype)


def clear_draws(cfg, sd, pix, K, c2w, S_mat, dists, mask, it, tables):
    """For the rays ``pix`` and K candidate tables [K, n, S]: (chosen [n, S] = index of the first candidate for which every
    appearance pre-activation of the row keeps MARGIN in float64, -1 if none; share [K] = fraction of clear rows among those
    each draw was tried on)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        n, s = tables.shape[1:]
        rec = _Recorder()
        ren = _SeamRenderer(rec, cfg)
        ren.seam = (dists, mask)
        net = o1.NeuralNetwork(cfg)
        net.load_state_dict(sd)
        net = net.double()
        worst = [None]

        def seen(mod, i, o):
            m = o.detach().abs().min(-1).values
            worst[0] = m if worst[0] is None else torch.minimum(worst[0], m)
        hooks = [getattr(net, 'lina%d' % l).register_forward_hook(seen) for l in range(net.n_app - 1)]
        chosen = torch.full((n * s,), -1, dtype=torch.long)
        todo = torch.arange(n * s)
        share = []
        for k in range(tables.shape[0]):
            if todo.numel() == 0:
                share.append(float('nan'))
                continue
            nz = {'full': tables[k].double(), 'nbr_full': torch.full((n, 3), 0.5)}
            with torch.no_grad():
                rec.p = None
                ren(pix[None].double(), K.double(), c2w.double(), S_mat.double(), 'unisurf', add_noise=True, eval_=False, it=it,
                    noise=group_noise(nz, mask))
            assert rec.p.shape[0] == n * s  # (one network call: row = ray * S + sample)
            worst[0] = None
            with torch.no_grad():
                net(rec.p[todo].clone(), rec.view[todo], return_addocc=True)
            ok = worst[0] >= MARGIN
            share.append(float(ok.double().mean()))
            chosen[todo[ok]] = k
            todo = todo[~ok]
        for h in hooks:
            h.remove()
        return chosen.reshape(n, s), share
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------ the cases
# name -> dict(N, it, seed, weights, over: configuration overrides, hits: None = the pool's own mix | exact number of hit rays,
#              normal / mask_loss / empty_norm: which terms the case enables, sd: weights seed, truth: the case whose reference /
#              truth it shares (the same step, run another way), trainer: targets from the planes of a stage1_batch)
# N is never a multiple of 4.  The seed of a case whose reference is more than 10 x further from float64 than ``default``'s is
# changed (tests/test_step1_grad_cpu.py asserts it); none needed another seed so far.
def _case(N=130, it=100, seed=300, weights=WEIGHTS, over=None, hits=None, normal=True, mask_loss=False, empty_norm=False, sd=11,
          truth=None, trainer=False):
    return dict(N=N, it=it, seed=seed, weights=tuple(weights), over=dict(over or {}), hits=hits, normal=normal, mask_loss=mask_loss,
                empty_norm=empty_norm, sd=sd, truth=truth, trainer=trainer)


CASES = {
    'default': _case(),
    'outer': _case(N=70, it=6000, seed=301),                 # S = 96: outer samples, composite flat layout 64 < S <= 128
    'shipped_weights': _case(weights=SHIPPED),               # (same rays and tables as default; its own truth)
    'n1_hit': _case(N=1, hits=1, seed=302),
    'n1_miss': _case(N=1, hits=0, seed=303),
    'n31': _case(N=31, seed=304),                            # 2 N = 62 / 66 normal rows: either side of a 64-row block
    'n33': _case(N=33, seed=305),
    'all_hit': _case(N=70, hits=70, seed=306),
    'all_miss': _case(N=70, hits=0, seed=307),
    'one_hit': _case(N=70, hits=1, seed=308),
    'mask_loss': _case(N=70, mask_loss=True, seed=309, weights=WEIGHTS[:3] + (0.04,)),  # (at 1.0 the BCE term is 90 % of the gradient)
    'no_normal_loss': _case(N=70, normal=False, seed=310),
    'empty_norm_mask': _case(N=70, empty_norm=True, seed=311),
    'white_bg': _case(N=70, over={'rendering.white_background': True}, seed=312),
    'reference_shaped': _case(truth='default'),
    'torch_glue': _case(truth='default'),
    'layerwise': _case(truth='default'),
    'chunked': _case(truth='default'),
    'h64': _case(N=70, over={'model.hidden_dim': 64, 'model.feat_size': 64}, seed=313),
    'ray_shards': _case(truth='default'),
    'trainer': _case(N=70, it=1000, seed=314, trainer=True),
}
# every other case renders on black: the bunny configuration ships white_background = True, which 'white_bg' keeps
for _k, _c in CASES.items():
    _c['over'].setdefault('rendering.white_background', False)
TRAINER_BATCH_SEED = 4


def trainer_cfg_overrides(ci):
    """The configuration overrides with which a Trainer runs the ``trainer`` case: its loss weights and ray count."""
    w = ci['weights']
    return dict(ci['over'], **{'training.lambda_l1_rgb': w[0], 'training.lambda_normals': w[1], 'training.lambda_normloss': w[2],
                               'training.lambda_mask': w[3], 'training.n_training_points': ci['pix'].shape[1]})


def _trainer_targets(cfg, data, pix, it):
    """training.py:166-191 with the oracle's helpers: what o1.Trainer.compute_loss hands to the loss."""
    import numpy as np
    tr = cfg['training']
    norm_mask = o1.gather_pixels(data['img.norm_mask'].unsqueeze(1), pix).bool().squeeze(-1)
    rgb_gt = o1.gather_pixels(data['img'], pix)
    assert tr['normal_loss'] and it >= tr['normal_after']
    normal_gt = o1.gather_pixels(data['img.normal'], pix)
    cos_t = np.cos(np.deg2rad(tr['normal_angle']))
    assert float((normal_gt[..., -1] - cos_t).abs().min()) > 1e-4, 'a target normal sits on the angle threshold'
    norm_mask[normal_gt[..., -1] < cos_t] = False
    flip = torch.tensor([[[1, -1, -1]]], dtype=torch.float32)
    normal_gt = torch.einsum('bij,bnj->bni', data['img.world_mat'][:, :3, :3] * flip, normal_gt)
    return rgb_gt, normal_gt, norm_mask


def case_inputs(name):
    """The finished case (see the module docstring), all from its seeds (CPU)."""
    c = CASES[name]
    assert c['truth'] is None
    cfg = stage1_cfg('bunny', **c['over'])
    sd = stage1_state_dict(cfg, seed=c['sd'])
    K, c2w, S_mat = stage1_camera(cfg, h=H, w=W)
    pl = pool(c['over'], c['sd'])
    g = torch.Generator().manual_seed(c['seed'])
    el = pl['eligible'].nonzero()[:, 0]
    order = el[torch.randperm(el.numel(), generator=g)]
    n, n_samples = c['N'], (96 if c['it'] > 5000 else 64)
    if c['hits'] is None:
        cand = order[:n + SPARE]
    else:
        oh, om = order[pl['mask'][order]], order[~pl['mask'][order]]
        cand = torch.cat([oh[:c['hits'] + (SPARE if c['hits'] else 0)], om[:n - c['hits'] + (SPARE if n > c['hits'] else 0)]])
        pos = {int(r): i for i, r in enumerate(order)}
        cand = torch.tensor(sorted((int(r) for r in cand), key=pos.get), dtype=torch.long)  # the pool's own interleaving
    tables = torch.rand(K_DRAWS, cand.numel(), n_samples, generator=g)
    chosen, share = clear_draws(cfg, sd, pl['pix'][cand], K, c2w, S_mat, pl['dists'][cand], pl['mask'][cand], c['it'], tables)
    good = (chosen >= 0).all(1)
    keep, replaced, left = [], 0, {True: c['hits'], False: None if c['hits'] is None else n - c['hits']}
    for i in range(cand.numel()):
        is_hit = bool(pl['mask'][cand[i]])
        if len(keep) == n or (c['hits'] is not None and left[is_hit] == 0):
            continue
        if not bool(good[i]):
            replaced += 1
            continue
        keep.append(i)
        if c['hits'] is not None:
            left[is_hit] -= 1
    assert len(keep) == n, '%s: only %d of %d rays with a clear draw in every row' % (name, len(keep), n)
    keep = torch.tensor(keep, dtype=torch.long)
    rays = cand[keep]
    full = torch.gather(tables[:, keep].permute(1, 2, 0), 2, chosen[keep].unsqueeze(-1)).squeeze(-1).contiguous()
    mask = pl['mask'][rays].clone()
    assert c['hits'] is None or int(mask.sum()) == c['hits']
    ci = dict(over=c['over'], sd=sd, pix=pl['pix'][rays][None].contiguous(), K=K, c2w=c2w, S=S_mat, dists=pl['dists'][rays].clone(),
              mask=mask, it=c['it'], noise={'full': full, 'nbr_full': torch.rand(n, 3, generator=g)}, weights=c['weights'],
              clear_share=share, replaced=replaced, depth_diff=pl['depth_diff'], pool_eligible=int(el.numel()))
    # (b) targets, placed clear of the L1 kinks of the float64 forward
    if c['trainer']:
        data = stage1_batch(cfg, h=H, w=W, seed=TRAINER_BATCH_SEED)
        ci['data'] = data
        rgb_gt, normal_gt, norm_mask = _trainer_targets(cfg, data, ci['pix'], c['it'])
    else:
        rgb_gt = torch.rand(1, n, 3, generator=g)
        normal_gt = torch.nn.functional.normalize(torch.randn(1, n, 3, generator=g), dim=-1)
        norm_mask = torch.rand(1, n, generator=g) > 0.3
    if c['empty_norm']:
        norm_mask = torch.zeros(1, n, dtype=torch.bool)
    # mask_gt: 1 on every hit ray, both values on the miss rays.  A hit ray with mask_gt = 0 would put 1 / (1 - acc) with
    # 1 - acc ~ 1e-4 into the gradient: a cancellation that no fp32 evaluation resolves (the reference sat 8e-3 from float64
    # with such labels), i.e. a badly conditioned input, not a property of any implementation.
    mask_gt = torch.where(pl['mask'][rays][None], torch.ones(1, n), (torch.rand(1, n, generator=g) > 0.5).float())
    ci.update(rgb_gt=rgb_gt, normal_gt=None, norm_mask=None, mask_gt=None, mask_valid=None)
    probe = {}
    with torch.no_grad():  # (one float64 forward; the oracle's gradient() re-enables the graph it needs inside)
        step_gradients(torch.float64, c['over'], sd, ci, probe=probe, forward_only=True)
    ci['pre_min'] = float(probe['pre_min'].min())
    assert ci['pre_min'] >= MARGIN, '%s: a row of the finished case is not clear (%.2e)' % (name, ci['pre_min'])

    def nudge(target, value, rows):
        close = ((value - target.double()).abs() < 2 * MARGIN) & rows
        assert not (c['trainer'] and bool(close.any())), '%s: a target of the batch sits on an L1 kink: another batch seed' % name
        target = torch.where(close, target + 8 * MARGIN, target)
        assert bool((((value - target.double()).abs() >= MARGIN) | ~rows).all())
        return target
    ci['rgb_gt'] = nudge(rgb_gt, probe['rgb'], torch.ones(1, 1, 1, dtype=torch.bool))
    if c['normal']:
        ci['norm_mask'] = norm_mask
        ci['normal_gt'] = nudge(normal_gt, probe['normal_pred'], norm_mask.unsqueeze(-1))
    if c['mask_loss']:
        acc = probe['acc_map']
        ci['mask_gt'] = mask_gt
        ci['mask_valid'] = ((torch.arange(n) % 5 != 0)[None] & (acc > MARGIN) & (acc < 1 - MARGIN))
        assert int(ci['mask_valid'].sum()) > n // 2 and 0 < float(mask_gt[ci['mask_valid']].mean()) < 1
    return ci


_CACHE = {}


def case_data(name):
    """(inputs, ref, truth) of a case: the restated step at fp32 and at float64, computed once per process and shared by every
    test that needs them (and by the cases that run the same step another way).  Treat all three as read-only."""
    key = CASES[name]['truth'] or name
    if key not in _CACHE:
        if key == 'shipped_weights':  # default's rays, tables and targets at the shipped weights
            ci = dict(case_data('default')[0], weights=CASES[key]['weights'])
        else:
            ci = case_inputs(key)
        ref = step_gradients(torch.float32, ci['over'], ci['sd'], ci)
        truth = step_gradients(torch.float64, ci['over'], ci['sd'], ci)
        _CACHE[key] = (ci, ref, truth)
    return _CACHE[key]


GEOMETRY = tuple('lin%d.%s' % (l, p) for l in range(9) for p in ('weight_g', 'weight_v', 'bias'))


def term_shares(name):
    """(d): {term: (share, tensor)} in float64 -- per loss term the case enables, the largest max|weight x that term's gradient|
    / max|gradient| over the geometry tensors (the gradient is linear in the weights: one backward per term)."""
    ci, _, truth = case_data(name)
    out = {}
    for i, term in enumerate(('rgb', 'smooth', 'normal', 'mask')):
        if ci['weights'][i] == 0 or (term == 'normal' and ci['normal_gt'] is None) or (term == 'mask' and ci['mask_gt'] is None):
            continue
        w = [0.0] * 4
        w[i] = ci['weights'][i]
        g = step_gradients(torch.float64, ci['over'], ci['sd'], ci, weights=w)
        best = max(((float(g[k].abs().max()) / float(truth[k].abs().max()), k) for k in truth if k in GEOMETRY and float(truth[k].abs().max()) > 0),
                   default=(0.0, ''))
        out[term] = best
    return out
