"""The stage-2 train step's gradients, parameter by parameter, against float64: cases, truth, reference and gate (no GPU).

``step_gradients`` restates the oracle's step body (oracle/stage2.py TrainStep.step + train_fix) in ONE dtype: light tables ->
rows l_slt -> normalise -> o2.PSNetwork -> o2.MainLoss + o2.NormalLoss -> backward.  At float32 it IS the reference arithmetic
(tests/test_step_grad_cpu.py anchors it to o2.TrainStep's own gradients); at float64, with the fp32 weights, inputs and jitter
draws cast up, it is the exact value of the reference formulas for those inputs (the truth, as helpers.stage2_truth is for outputs).

``check(hip, ref, truth, what)`` is the gate.  Per gradient tensor, s = max|truth|:
  tensor form  e_t(x) = max|x - truth| / s
  row form     (tensors of >= 2 dimensions) e_r(x) = max over the rows r of dimension 0 with max|truth_r| >= 1e-3 s of
               max|x_r - truth_r| / max|truth_r|   (smaller rows are covered by the tensor form)
E_t / E_r = the worst e_t(ref) / e_r(ref) over ALL tensors of the case (one small tensor's own figure can be lucky by 100 x;
the case-wide worst is stable), and every tensor of ``hip`` must satisfy e_t <= 8 E_t and e_r <= 8 E_r: 2 for two independent
fp32 roundings of the same formulas (helpers.truth_ratios) x 4 for the product regrouping nearly every sum of the chain (split-K
over the V Ns rows, 4-deep MFMA accumulation steps, per-block partials of the loss and pair-sum kernels, init-table products
formed once per table row; the CPU reference uses FMA-blocked GEMMs and pairwise sums).  The factor is fixed against reference
and truth, never against the kernels.  A tensor whose truth is all zero must be all zero or absent; a gradient the truth does not
have (a frozen parameter) must be None or exactly zero; the sets of names must agree; a NaN never passes.

The cases (CASES) are built from seeds; their surface pixels are drawn from the pixels that are clear of every kink of the step
(pixel_margins, MARGIN): on a kink no two fp32 evaluations agree, the reference's own included.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import stage2 as o2
from psnerf_amd.synthetic import stage2_inputs
from tests.helpers import stage2_state_dict

FACTOR = 8.0          # see the module docstring
ROW_FLOOR = 1e-3      # rows below ROW_FLOOR * max|truth| are judged by the tensor form only
PHASE_WEIGHTS = {1: dict(sg_rgb_weight=0, albedo_smooth_weight=0, rough_smooth_weight=0, vis_weight=10),   # train_fix at iteration 0
                 2: dict(sg_rgb_weight=1.0, albedo_smooth_weight=0.05, rough_smooth_weight=0.01, vis_weight=1)}
NORMAL_WEIGHTS = dict(normal_weight=1, normal_smooth_weight=0.05)
PIXEL_KEYS = ('uv', 'object_mask', 'surface_mask', 'points', 'normal', 'vis_train_gt', 'visibility')


# ------------------------------------------------------------------------------------------------ the restated step
def _up(v, dtype):
    if isinstance(v, dict):
        return {k: _up(x, dtype) for k, x in v.items()}
    if torch.is_tensor(v):
        v = v.detach().cpu()
        return v.to(dtype) if v.dtype == torch.float32 else v
    return v


MUTANTS = ('vis_w', 'rgb_w', 'rough_w', 'albedo_w', 'no_jitter_half', 'drop_row', 'masked_pixel')


def step_gradients(dtype, conf_overrides, state_dict, batch, l_slt, noise, phase, loss_type, light_init=None, mutant=None):
    """{name: float64 tensor} of every trainable parameter's gradient (+ '__light_dir' / '__light_int', the dense table
    gradients, when the tables train) of ONE stage-2 step evaluated in ``dtype``; {} when the loss has no graph (no surface
    pixel).  batch = (model_input, ground_truth); light_init [n_lights_total, 3] = the direction table (= the frozen initial
    estimates the supervision lights are taken from, trainer.py:149,377).  ``mutant``: one deliberate error (MUTANTS), used
    only to show that the gate can fail."""
    assert mutant is None or mutant in MUTANTS, mutant
    conf = o2.bear_conf(**conf_overrides)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)  # the oracle allocates its dense outputs with the default dtype
    try:
        model = o2.PSNetwork(conf)
        model.load_state_dict(state_dict)
        model = model.to(dtype)
        inp, gt = _up(batch[0], dtype), _up(batch[1], dtype)
        inp.pop('surface_idx', None)
        inp.pop('surface_count', None)
        noise = _up(noise or {}, dtype)
        lw = dict(PHASE_WEIGHTS[phase])
        nw = dict(NORMAL_WEIGHTS)
        for key, name, f in (('vis_w', 'vis_weight', 0.999), ('rgb_w', 'sg_rgb_weight', 0.999),
                             ('rough_w', 'rough_smooth_weight', 0.99), ('albedo_w', 'albedo_smooth_weight', 0.99)):
            if mutant == key:
                lw[name] = lw[name] * f
        loss_main, loss_n = o2.MainLoss(loss_type=loss_type, **lw), o2.NormalLoss(**nw)
        # the switches of TrainStep.__init__ and the state train_fix leaves behind in this phase
        light_train = conf.get_bool('train.light_train', default=False)
        inten_train = light_train and conf.get_bool('train.light_inten_train', default=False)
        visibility = conf.get_bool('train.visibility', default=False)
        vis_loss = visibility and conf.get_bool('train.vis_loss', default=False)
        normal_train = conf.get_bool('train.normal_mlp', default=False) and conf.get_bool('train.normal_joint', default=False)
        if phase == 1:
            model.albedo_net.eval().requires_grad_(False)
            model.rough_net.eval().requires_grad_(False)
        if visibility and not vis_loss:
            model.visibility_net.eval().requires_grad_(False)
        tables_train = light_train and phase == 2 and not conf.get_bool('train.ana_fixlight', default=False)
        light_dir = light_int = None
        if light_train:
            light_dir = light_init.detach().clone().to(dtype).requires_grad_(tables_train)
            inp['light_direction'] = F.normalize(light_dir[l_slt], p=2, dim=-1)
            if inten_train:
                light_int = torch.full((light_init.shape[0], 1), model.light_int, dtype=dtype).requires_grad_(tables_train)
                inp['light_intensity'] = light_int[l_slt]
            if 'light_vis_train' not in inp:
                inp['light_vis_train'] = F.normalize(light_init.detach().to(dtype)[l_slt], p=2, dim=-1)
        if not bool(inp['surface_mask'].any()):
            # no pixel on the surface: every output is a constant and every loss term the constant 0 (loss.py:20-24), so no
            # parameter has a gradient.  (The reference's forward cannot run this batch at all: renderer.py:251-262 reads the
            # point encoding that only exists with surface pixels.)
            return {}
        out = model(inp, noise=noise)
        scale = 1.0
        if mutant == 'no_jitter_half':
            out['albedo_jitter'], out['rough_jitter'] = out['albedo_jitter'].detach(), out['rough_jitter'].detach()
        elif mutant == 'drop_row':  # the first pixel the losses see contributes nothing to the backward pass
            m = out['network_object_mask'] & out['object_mask']
            one = torch.zeros_like(m)
            one[0, int(m[0].nonzero()[0])] = True
            for k, v in list(out.items()):
                if torch.is_tensor(v) and v.requires_grad:
                    out[k] = torch.where(one.expand(v.shape[0], -1).unsqueeze(-1), v.detach(), v)
        elif mutant == 'masked_pixel':  # a surface pixel outside the object mask enters the sums (same normalisation)
            m = out['network_object_mask'] & ~out['object_mask']
            before = int((out['network_object_mask'] & out['object_mask']).sum())
            om = out['object_mask'].clone()
            om[0, int(m[0].nonzero()[0])] = True
            out['object_mask'] = om
            scale = (before + 1.0) / before  # every term is a mean over (count x constant): undo the change of the count
        terms = loss_main(out, gt, inp)
        loss = terms['loss']
        if normal_train:
            loss = loss + loss_n(out)['loss']
        loss = loss * scale if scale != 1.0 else loss
        if not loss.requires_grad:
            return {}
        loss.backward()
        grads = {k: p.grad.detach().double() for k, p in model.named_parameters() if p.requires_grad and p.grad is not None}
        if tables_train:
            grads['__light_dir'] = light_dir.grad.detach().double()
            if inten_train:
                grads['__light_int'] = light_int.grad.detach().double()
        return grads
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------ the gate
def _np(x):
    return np.asarray(x.detach().cpu().double() if torch.is_tensor(x) else x, dtype=np.float64)


def figures(x, truth):
    """(e_t, e_r) of one tensor against its (non-zero) truth; e_r is None for 1-D tensors and when no row reaches the floor.
    A NaN anywhere gives inf."""
    x, t = _np(x), _np(truth)
    assert x.shape == t.shape, 'shape %s vs %s' % (x.shape, t.shape)
    s = float(np.abs(t).max())
    d = np.abs(x - t)
    d = np.where(np.isnan(d), np.inf, d)
    e_t = float(d.max()) / s
    e_r = None
    if t.ndim >= 2:
        tr = np.abs(t).reshape(t.shape[0], -1).max(1)
        rows = tr >= ROW_FLOOR * s
        if rows.any():
            e_r = float((d.reshape(t.shape[0], -1).max(1)[rows] / tr[rows]).max())
    return e_t, e_r


def measure(hip, ref, truth):
    """Every figure and every violation of the gate, without asserting: dict(E_t, E_r, hip_t, hip_r, hip_t_name, hip_r_name,
    ref_t_name, ref_r_name, bad=[messages])."""
    hip = {k: v for k, v in hip.items() if v is not None}
    bad = []
    E_t = E_r = 0.0
    n_t = n_r = ''
    live = []
    for k in sorted(truth):
        t = _np(truth[k])
        assert k in ref, 'the reference has no gradient for %s' % k
        if not np.isfinite(t).all():
            bad.append('%s: the truth is not finite' % k)
            continue
        if float(np.abs(t).max()) == 0.0:  # rule 2
            for tag, d in (('hip', hip), ('ref', ref)):
                if k in d and not (_np(d[k]) == 0.0).all():
                    bad.append('%s: truth is all zero, %s is not' % (k, tag))
            continue
        live.append(k)
        e_t, e_r = figures(ref[k], t)
        if e_t > E_t:
            E_t, n_t = e_t, k
        if e_r is not None and e_r > E_r:
            E_r, n_r = e_r, k
    for k in sorted(set(ref) - set(truth)):
        if not (_np(ref[k]) == 0.0).all():
            bad.append('%s: the reference has a gradient the truth does not have' % k)
    for k in sorted(set(hip) - set(truth)):  # rule 3
        if not (_np(hip[k]) == 0.0).all():
            bad.append('%s: a gradient the truth does not have (frozen parameter) is not zero' % k)
    h_t = h_r = 0.0
    hn_t = hn_r = ''
    for k in live:
        if k not in hip:
            bad.append('%s: no gradient' % k)
            continue
        if tuple(_np(hip[k]).shape) != tuple(_np(truth[k]).shape):
            bad.append('%s: shape %s, truth %s' % (k, tuple(_np(hip[k]).shape), tuple(_np(truth[k]).shape)))
            continue
        e_t, e_r = figures(hip[k], truth[k])
        if not e_t <= FACTOR * E_t:
            bad.append('%s: e_t = %.3e > %g x E_t = %.3e' % (k, e_t, FACTOR, FACTOR * E_t))
        if e_r is not None and not e_r <= FACTOR * E_r:
            bad.append('%s: e_r = %.3e > %g x E_r = %.3e' % (k, e_r, FACTOR, FACTOR * E_r))
        if e_t > h_t:
            h_t, hn_t = e_t, k
        if e_r is not None and e_r > h_r:
            h_r, hn_r = e_r, k
    return dict(E_t=E_t, E_r=E_r, hip_t=h_t, hip_r=h_r, hip_t_name=hn_t, hip_r_name=hn_r, ref_t_name=n_t, ref_r_name=n_r,
                n_tensors=len(live), bad=bad)


def report_line(what, m, prefix='step-grad'):
    rt = m['hip_t'] / (FACTOR * m['E_t']) if m['E_t'] > 0 else float('nan')
    rr = m['hip_r'] / (FACTOR * m['E_r']) if m['E_r'] > 0 else float('nan')
    return ('%s %-18s tensors %2d | E_t %.2e (%s) E_r %.2e (%s) | hip e_t %.2e = %.2f of allowance (%s) | hip e_r %.2e = %.2f of allowance (%s)'
            % (prefix, what, m['n_tensors'], m['E_t'], m['ref_t_name'], m['E_r'], m['ref_r_name'], m['hip_t'], rt, m['hip_t_name'],
               m['hip_r'], rr, m['hip_r_name']))


def check(hip, ref, truth, what, prefix='step-grad'):
    """The gate of the module docstring; prints one line per case and returns the figures."""
    m = measure(hip, ref, truth)
    print(report_line(what, m, prefix))
    assert not m['bad'], '%s: %d violation(s) of the gradient gate:\n  %s' % (what, len(m['bad']), '\n  '.join(m['bad']))
    return m


# ------------------------------------------------------------------------------------------------ well-conditioned pixels
# The step is piecewise smooth: every ReLU, clamp, |.| of an L1 term and GGX indicator is a kink, and a pixel that sits ON one
# has no gradient any fp32 evaluation could agree on -- the reference arithmetic flips such a decision as readily as a kernel.
# Measured in the reference arithmetic (fp32 oracle against its float64 evaluation, 270 surface pixels, bear configuration): the
# largest pre-activation difference is 4.5e-6, about twenty units per batch lie within 1e-6 of zero, and ONE flipped ReLU moves
# a weight row's gradient by 1e-2 of its size -- 1000 x the rounding the gate is built on.  So the surface pixels of every case
# are DRAWN FROM THOSE WHOSE EVERY DECISION IS CLEAR in float64: each quantity a kink compares with a constant keeps MARGIN from
# it.  MARGIN = 2e-5 is four times the largest fp32 pre-activation error seen in the reference arithmetic, and comes from that
# alone.  Pixels are independent of each other, so this is a property of a pixel (given weights, lights and its jitter draw).
MARGIN = 2e-5


def pixel_margins(conf_overrides, state_dict, inp, gt, noise):
    """Per pixel [N] float64: the smallest distance of any kink quantity from its kink, with EVERY pixel of ``inp`` treated as a
    surface pixel inside the object mask.  ``inp`` carries the lights the model will see ('light_direction', 'light_vis_train'
    if any); noise: {'xyz' [N, 3], 'normal' [N, 3]} per pixel."""
    conf = o2.bear_conf(**conf_overrides)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        model = o2.PSNetwork(conf)
        model.load_state_dict(state_dict)
        model = model.double()
        inp, gt, noise = _up(inp, torch.float64), _up(gt, torch.float64), _up(noise, torch.float64)
        n = inp['points'].shape[1]
        inp['surface_mask'] = torch.ones(1, n, dtype=torch.bool)
        inp['object_mask'] = torch.ones(1, n, dtype=torch.bool)
        worst = torch.full((n,), float('inf'))

        def near(x, *kinks):  # x: [..., n, C] or [rows = k n, C] (light-major); distance to the nearest kink value, per pixel
            x = x.detach()
            d = torch.stack([(x - k).abs() for k in kinks]).min(0).values
            d = d.reshape(-1, n, d.shape[-1])
            worst.copy_(torch.minimum(worst, d.min(-1).values.min(0).values))

        hooks = [m.register_forward_hook(lambda mod, i, o: near(o, 0.0)) for m in model.modules() if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            out = model(inp, noise=noise)
        for h in hooks:
            h.remove()
        ld = inp['light_direction']
        normal = out['normal_pred'][0] if 'normal_pred' in out else inp['normal'][0]
        cos = torch.einsum('li,ni->ln', ld, normal).unsqueeze(-1)                       # [L, n, 1]
        vis = out['visibility'].reshape(ld.shape[0], n, 3)[..., :1] if 'visibility' in out else torch.ones_like(cos)
        near(vis, 0.0, 1.0)                                                              # clamp(vis, 0, 1); |vis - gt| with gt in {0, 1}
        if 'vis_train' in out:
            near(out['vis_train'].reshape(-1, n, 3)[..., :1], 0.0, 1.0)
        near(cos, 0.0)
        light_int = inp.get('light_intensity', model.light_int)
        albedo = out['sg_diffuse_albedo_values'][0]
        if model.render_model == 'sgbasis':
            brdf = albedo[None] + out['sg_specular_rgb_values'].reshape(ld.shape[0], n, 3)
        else:  # GGX: the indicators and absolute values of model/microfacet.py on h.n, n.v, h.v
            rays, _ = o2.camera_rays(inp['uv'], inp['pose'], inp['intrinsics'])
            v = -rays[0]
            rough = out['sg_specular_rgb_values'][0][:, :1]
            brdf = o2.microfacet_brdf(ld[None].expand(n, -1, -1), v, normal, albedo, rough, f0=model.f0).permute(1, 0, 2)
            h = F.normalize(ld[:, None] + v[None], dim=-1)
            near((h * F.normalize(normal, dim=-1)[None]).sum(-1, keepdim=True), 0.0)
            near((h * v[None]).sum(-1, keepdim=True), 0.0)
            near((F.normalize(normal, dim=-1) * v).sum(-1, keepdim=True), 0.0, 1.0, -1.0)
        x = brdf * (light_int if not torch.is_tensor(light_int) else light_int.reshape(-1, 1, 1)) * cos * vis.clamp(0, 1)
        near(x, 0.0, 1.0)                                                                # the outer clamp of the colour
        near(out['sg_rgb_values'].reshape(ld.shape[0], n, 3) - gt['rgb'].reshape(ld.shape[0], n, 3), 0.0)
        for a, b in (('albedo_values', 'albedo_jitter'), ('rough_values', 'rough_jitter'), ('normal_pred', 'normal_jitter')):
            if a in out and b in out:
                d = (out[a] - out[b]).detach()
                both_off = (out[a] == 0) & (out[b] == 0)  # two clamped SG weights: |0 - 0| has the same (zero) gradient in every evaluation
                near(torch.where(both_off, torch.ones_like(d), d), 0.0)
        return worst
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------ the cases
def _mask_edge(inp):
    """object_mask false on every tenth surface pixel: their rows run forward and must add nothing to the gradients."""
    idx = inp['surface_mask'][0].nonzero(as_tuple=True)[0][::10]
    om = inp['object_mask'].clone()
    om[0, idx] = False
    inp['object_mask'] = om


def _drop(*keys):
    def edit(inp):
        for k in keys:
            inp.pop(k, None)
    return edit


# name -> dict(over: configuration overrides, phase, loss, N, Ns, L, V, NL, sd: state-dict seed, seed: batch seed,
#              pool: candidate pixels per batch pixel (tests/test_step_grad_cpu.py prints the fraction of clear ones),
#              pre: edit of the pixel pool (keys a configuration's batches do not carry), edit: edit of the finished batch,
#              truth: the case whose reference / truth it shares (the same step, run another way))
# N is never a multiple of 4; Ns walks through 1, the 64-row blocks of the engines (63 / 64 / 65), 129 and 541.
def _case(over=None, phase=2, loss='L1', N=602, Ns=541, L=3, V=2, NL=8, sd=5, seed=100, pre=None, edit=None, truth=None, pool=8):
    return dict(over=dict(over or {}), phase=phase, loss=loss, N=N, Ns=Ns, L=L, V=V, NL=NL, sd=sd, seed=seed, pre=pre, edit=edit,
                truth=truth, pool=pool)


CASES = {
    'default': _case(),
    'ns1': _case(N=5, Ns=1, seed=101),
    'ns63': _case(N=70, Ns=63, seed=102),
    'ns64': _case(N=71, Ns=64, seed=103),
    'ns65': _case(N=73, Ns=65, seed=104),
    'ns129': _case(N=150, Ns=129, seed=105, L=7, V=3, NL=12, pool=96),  # (ten lights: 2 % of the pixels are clear)
    'one_light': _case(N=150, Ns=129, seed=106, L=1, V=1),
    'phase1': _case(phase=1),
    'mask_edge': _case(edit=_mask_edge),
    'no_surface': _case(N=150, Ns=0, seed=107),
    'surface_idx': _case(truth='default'),
    'padded_count': _case(truth='default'),
    'padded': _case(truth='default'),
    'normal_jitter': _case({'normal.net.xyz_jitter_std': 0.02}, N=301, Ns=270, seed=108),
    'no_brdf_jitter': _case({'brdf.net.xyz_jitter_std': 0.0}, N=301, Ns=270, seed=109),
    'mono_specular': _case({'train.specular_rgb': False}, N=301, Ns=270, seed=110),
    'microfacet': _case({'train.render_model': 'microfacet'}, N=301, Ns=270, seed=131),  # (seed 111: E_t = 3.6e-3 in normal_net, 1000 x the default case's -> another seed, as test_step_grad_cpu.py prescribes)
    'l2': _case(loss='L2', N=301, Ns=270, seed=112, V=1),
    'no_inten_table': _case({'train.light_inten_train': False}, N=301, Ns=270, seed=113),
    'given_lights': _case({'train.light_train': False}, N=301, Ns=270, seed=114, pre=_drop('light_vis_train', 'vis_train_gt')),
    'fixed_lights': _case({'train.ana_fixlight': True}, N=301, Ns=270, seed=115),
    'no_vis_loss': _case({'train.vis_loss': False}, N=301, Ns=270, seed=116, pre=_drop('light_vis_train', 'vis_train_gt', 'visibility')),
    'light_vis_attached': _case({'train.light_vis_detach': False}, N=301, Ns=270, seed=117),
    'vis_rgb_attached': _case({'train.vis_rgb_detach': False}, N=301, Ns=270, seed=118),
    # (each switch on its own changes the launches only; with both off the colour's gradient reaches the light directions
    #  through the visibility net and the encoding backward)
    'vis_both_attached': _case({'train.light_vis_detach': False, 'train.vis_rgb_detach': False}, N=301, Ns=270, seed=119),
    'no_overlap': _case({'train.overlap_small_nets': False}, truth='default'),
    'global_count': _case(truth='default'),
}


def sub_batch(inp, gt, idx):
    """The pixels ``idx`` of a batch (what a data-parallel rank receives)."""
    n = inp['uv'].shape[1]
    sub = {k: (v[:, idx].contiguous() if (k in PIXEL_KEYS and torch.is_tensor(v) and v.dim() >= 2 and v.shape[1] == n) else v)
           for k, v in inp.items()}
    return sub, {'rgb': gt['rgb'][:, idx].contiguous()}


def case_inputs(name):
    """dict(conf_overrides, sd, batch=(inp, gt), l_slt, noise, light_init, phase, loss_type, clear) of a case, all from its seeds
    (CPU): N pixels of a seeded pool of pool x N + 64, the Ns surface pixels among the CLEAR ones (pixel_margins >= MARGIN)."""
    c = CASES[name]
    over = {k: v for k, v in c['over'].items() if k != 'train.overlap_small_nets'}
    conf = o2.bear_conf(**over)
    sd = stage2_state_dict(conf, seed=c['sd'])
    P = c['pool'] * c['N'] + 64
    inp, gt = stage2_inputs(P, c['L'], c['V'], seed=c['seed'])
    inp.pop('light_intensity')  # the trainer's batches carry none: the table row or the model's scalar (trainer.py:378-379, renderer.py:202)
    if c['pre'] is not None:
        c['pre'](inp)
    g = torch.Generator().manual_seed(c['seed'] + 2000)
    light_init = F.normalize(torch.randn(c['NL'], 3, generator=g), dim=-1)
    light_init[:, 2] = light_init[:, 2].abs() + 0.2
    l_slt = torch.randperm(c['NL'], generator=g)[:c['L']]
    noise = {'xyz': torch.randn(P, 3, generator=g) * 0.01}
    if over.get('normal.net.xyz_jitter_std', 0.0) > 0:
        noise['normal'] = torch.randn(P, 3, generator=g) * over['normal.net.xyz_jitter_std']
    order = torch.randperm(P, generator=g)
    # the lights the model sees, as step_gradients forms them
    seen = dict(inp)
    if conf.get_bool('train.light_train', default=False):
        seen['light_direction'] = F.normalize(light_init[l_slt], p=2, dim=-1)
        seen.setdefault('light_vis_train', F.normalize(light_init[l_slt], p=2, dim=-1))
    clear = pixel_margins(over, sd, seen, gt, noise)[order] >= MARGIN
    surf = order[clear][:c['Ns']]
    assert surf.numel() == c['Ns'], '%s: only %d clear pixels in a pool of %d' % (name, surf.numel(), P)
    rest = order[~clear][:c['N'] - c['Ns']]
    assert rest.numel() == c['N'] - c['Ns']
    pix = torch.sort(torch.cat([surf, rest])).values
    is_surf = torch.zeros(P, dtype=torch.bool)
    is_surf[surf] = True
    inp['surface_mask'] = is_surf[None].clone()
    inp['object_mask'] = inp['object_mask'] | inp['surface_mask']
    inp, gt = sub_batch(inp, gt, pix)
    noise = {k: v[pix][is_surf[pix]] for k, v in noise.items()}
    if c['edit'] is not None:
        c['edit'](inp)
    return dict(conf_overrides=over, sd=sd, batch=(inp, gt), l_slt=l_slt, noise=noise, light_init=light_init,
                phase=c['phase'], loss_type=c['loss'], clear=float(clear.double().mean()))


_CACHE = {}


def case_data(name):
    """(inputs, ref, truth) of a case: the restated step at fp32 and at float64, computed once per process and shared by
    every test that needs them (and by the cases that run the same step another way).  Treat all three as read-only."""
    key = CASES[name]['truth'] or name
    if key not in _CACHE:
        ci = case_inputs(key)
        ref = step_gradients(torch.float32, *step_args(ci), light_init=ci['light_init'])
        truth = step_gradients(torch.float64, *step_args(ci), light_init=ci['light_init'])
        _CACHE[key] = (ci, ref, truth)
    return _CACHE[key]


def step_args(ci):
    return (ci['conf_overrides'], ci['sd'], ci['batch'], ci['l_slt'], ci['noise'], ci['phase'], ci['loss_type'])


