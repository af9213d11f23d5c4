"""Inputs and the float64 definition for the direct tests of the SG and GGX shading kernels (csrc/shade.hip): seeded cases that
sit on both sides of every clamp, the oracle's formulas evaluated with autograd in float64 ("truth") or float32 ("the reference
arithmetic"), and the mask of (light, point) pairs on which a float32 evaluation cannot be expected to take float64's side of a
discontinuity.  Plain data and reference code: nothing here touches a GPU.

Rows are light-major, (l, n) -> l * Ns + n, as stage2/model/renderer.py:174-204 and the kernels lay them out."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import stage2 as o2

F0 = 0.05
MARGIN_COLOUR = 1e-4   # |pre-clamp colour - {0, 1}|
MARGIN_CANCEL = 1e-4   # |sum_k w_k D_k| relative to sum_k |w_k| D_k
MARGIN_DOT = 1e-3      # GGX: |h.n|, |h.v|, |n.v|, |l.n| of the normalised vectors

# (Ns, L): one thread per point in 64-point workgroups (idle-lane tail at 1, 63, 65, 130, 257; 1, 2, 3 and 5 workgroups, so the
# light reduce, which strides the workgroup partials by 4, sees counts below, at and above its stride); the SG waves take the
# lights l = phase mod 4, so L < 4 leaves phases without a light; L = 17 gives 68 reduce outputs = a second reduce workgroup.
SHAPES = [(1, 1), (1, 5), (63, 2), (63, 17), (64, 4), (64, 1), (65, 5), (65, 3), (130, 17), (130, 2), (257, 3), (257, 17), (257, 4)]

# intensity: 'float' python scalar | 'one' [1,1] tensor | 'L1' [L,1] tensor;  vis: None | 'detached' | 'grad'
_SG_VARIANTS = [  # nb, specular_rgb, intensity, vis, g_spec
    (9, True, 'L1', 'grad', True), (1, False, 'float', None, False), (5, True, 'one', 'detached', True),
    (9, False, 'L1', 'grad', True), (9, True, 'float', 'grad', False), (5, False, 'one', None, True),
    (9, True, 'L1', 'grad', True), (1, True, 'L1', 'detached', False), (9, True, 'one', 'grad', True),
    (5, False, 'float', 'grad', True), (9, False, 'L1', 'grad', False), (5, True, 'L1', 'detached', True),
    (1, False, 'one', 'grad', True)]
_MF_VARIANTS = [  # intensity, vis
    ('L1', 'grad'), ('float', None), ('one', 'detached'), ('L1', 'grad'), ('float', 'grad'), ('one', None), ('L1', 'grad'),
    ('L1', 'detached'), ('one', 'grad'), ('float', 'grad'), ('L1', 'grad'), ('L1', 'detached'), ('one', 'grad')]

SG_CASES = [dict(kernel='sg', Ns=ns, L=l, nb=nb, specular_rgb=srgb, intensity=it, vis=vis, g_spec=gs, seed=100 + i)
            for i, ((ns, l), (nb, srgb, it, vis, gs)) in enumerate(zip(SHAPES, _SG_VARIANTS))]
MF_CASES = [dict(kernel='mf', Ns=ns, L=l, intensity=it, vis=vis, seed=200 + i)
            for i, ((ns, l), (it, vis)) in enumerate(zip(SHAPES, _MF_VARIANTS))]
# [L,3] RGB lights (stage2/eval.py:200): forward only
SG_RGB_LIGHT_CASES = [dict(kernel='sg', Ns=65, L=5, nb=9, specular_rgb=True, intensity='L3', vis='detached', g_spec=False, seed=150),
                      dict(kernel='sg', Ns=130, L=17, nb=5, specular_rgb=False, intensity='L3', vis=None, g_spec=False, seed=151)]


def case_id(spec):
    if spec['kernel'] == 'sg':
        return 'sg-%dx%d-nb%d-%s-I%s-vis%s-%s' % (spec['Ns'], spec['L'], spec['nb'], 'rgb' if spec['specular_rgb'] else 'mono',
                                                  spec['intensity'], spec['vis'], 'gspec' if spec['g_spec'] else 'nogspec')
    return 'mf-%dx%d-I%s-vis%s' % (spec['Ns'], spec['L'], spec['intensity'], spec['vis'])


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _visibility(g, n):
    """[0.1, 0.9], below 0, above 1, and the two values at which the inclusive clamp backward is decided exactly."""
    kind = g.choice(5, size=n, p=[0.56, 0.12, 0.12, 0.10, 0.10])
    return np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                     [g.uniform(0.1, 0.9, n), g.uniform(-0.5, -0.01, n), g.uniform(1.01, 1.5, n), np.zeros(n)], np.ones(n))


def draw_inputs(spec):
    """The raw float32 inputs of a case (no upstream gradients yet) as a dict of CPU tensors / python values."""
    g = np.random.RandomState(spec['seed'])
    Ns, L, mf = spec['Ns'], spec['L'], spec['kernel'] == 'mf'
    n_hat = _unit(g.standard_normal((Ns, 3)))
    view = _unit(n_hat + 0.6 * g.standard_normal((Ns, 3)))          # the normal's hemisphere plus noise
    light = _unit(g.standard_normal((L, 3)))                         # the whole sphere: ~40 % of the pairs are back-facing
    if mf:   # the kernel normalises all three and carries the adjoints
        normal = n_hat * g.uniform(0.5, 2.0, (Ns, 1))
        view = view * g.uniform(0.5, 2.0, (Ns, 1))
        light = light * g.uniform(0.5, 2.0, (L, 1))
    else:    # |n| > 1 would make h.n - 1 > 0 and the e^10 lobe overflow in the reference as well
        normal = n_hat * g.uniform(0.9, 1.0, (Ns, 1))
    c = dict(spec)
    c.update(light_dir=light, view=view, normal=normal, albedo=g.uniform(0.05, 0.95, (Ns, 3)))
    if mf:
        c['rough'] = g.uniform(0.05, 0.95, (Ns, 1))
        lo, hi = 3.0, 12.0   # albedo / pi <= 0.3: the upper colour clamp needs this much light
    else:
        nb = spec['nb']
        c['weights'] = 0.6 * g.standard_normal((Ns, nb * (3 if spec['specular_rgb'] else 1)))   # both signs: the specular clamp
        lobe = np.exp(2.0 + np.arange(nb))
        if nb > 2:
            lobe[1] = -3.0   # lobe.clamp(min=0) -> lambda = 0, D = 1
        c['lobe'] = lobe
        lo, hi = 1.0, 6.0
    kind = spec['intensity']
    if kind == 'float':
        c['light_int'] = float(np.float32(0.5 * (lo + hi)))
    else:
        shape = {'one': (1, 1), 'L1': (L, 1), 'L3': (L, 3)}[kind]
        c['light_int'] = g.uniform(0.5 * (lo + hi) if kind == 'one' else lo, hi, shape)   # one light level: the upper half
    c['vis_in'] = None if spec['vis'] is None else _visibility(g, L * Ns).reshape(L * Ns, 1)
    c['g_rgb'] = g.standard_normal((L * Ns, 3))
    if not mf:
        c['g_spec_in'] = g.standard_normal((L * Ns, 3 if spec['specular_rgb'] else 1)) if spec['g_spec'] else None
    for k, v in list(c.items()):
        if isinstance(v, np.ndarray):
            c[k] = torch.from_numpy(v.astype(np.float32))   # float32 FIRST: both precisions then see identical values
    return c


def _rows(c, dtype, leaves=False):
    """The case's tensors in ``dtype`` (cast up from float32) -> dict; leaves: those a gradient is asked for require it."""
    t = {}
    for k in ('light_dir', 'view', 'normal', 'albedo', 'weights', 'rough', 'lobe', 'vis_in', 'light_int'):
        v = c.get(k)
        if torch.is_tensor(v):
            v = v.detach().to(dtype).clone()
            if leaves and k not in ('view', 'lobe'):
                v.requires_grad_(True)
        t[k] = v
    return t


def sg_brdf(l, v, n, albedo, weights, lobe, specular_rgb):
    """oracle.stage2.SGBasis on rows, with the case's lobe vector in place of exp(2..10) -> (brdf [R,3], spec [R,3 or 1])."""
    sg = o2.SGBasis(nbasis=int(lobe.shape[0]), specular_rgb=bool(specular_rgb))
    sg.lobe = torch.nn.Parameter(lobe.detach().clone(), requires_grad=False)
    return sg(v=v, n=n, l=l, albedo=albedo, weights=weights)


def mf_brdf(pts2l, v, n, albedo, rough, f0=F0):
    """oracle.stage2.microfacet_brdf: pts2l [N,L,3] -> [N,L,3]."""
    return o2.microfacet_brdf(pts2l, v, n, albedo, rough, f0=f0)


def forward(c, t):
    """The reference forward on the tensors ``t`` of _rows(): the BRDF, then the render line of oracle/stage2.py:277-288 (cos = l.n
    on the raw inputs, un-clamped; brdf * I * cos * vis.clamp(0, 1); .clamp(0, 1)).  -> dict rgb, pre (pre-clamp colour), spec."""
    L, Ns = c['L'], c['Ns']
    pts2l = t['light_dir'][:, None].expand(L, Ns, 3).reshape(-1, 3)
    out = {}
    if c['kernel'] == 'sg':
        brdf, out['spec'] = sg_brdf(pts2l, t['view'].tile(L, 1), t['normal'].tile(L, 1), t['albedo'].tile(L, 1),
                                    t['weights'].tile(L, 1), t['lobe'], c['specular_rgb'])
    else:
        brdf = mf_brdf(pts2l.view(L, -1, 3).permute(1, 0, 2), t['view'], t['normal'], t['albedo'], t['rough']
                       ).permute(1, 0, 2).reshape(-1, 3)
    cos = torch.einsum('lni,ni->ln', pts2l.view(L, -1, 3), t['normal']).reshape(-1, 1)
    light_int = t['light_int']
    if torch.is_tensor(light_int) and light_int.shape[0] > 1:
        light_int = light_int.repeat_interleave(Ns, dim=0)
    pre = brdf * light_int * cos
    if t['vis_in'] is not None:
        pre = pre * t['vis_in'].clamp(0, 1)
    out['pre'], out['rgb'] = pre, pre.clamp(0, 1)
    return out


def ambiguous_pairs(c):
    """bool [L*Ns], decided in float64: pairs whose float64 value sits on a discontinuity (module docstring).  Also returns the
    float64 quantities the coverage conditions are stated on."""
    L, Ns = c['L'], c['Ns']
    t = _rows(c, torch.float64)
    with torch.no_grad():
        out = forward(c, t)
        pre = out['pre']
        vcl0 = (t['vis_in'].clamp(0, 1) == 0).reshape(-1) if t['vis_in'] is not None else torch.zeros(L * Ns, dtype=torch.bool)
        near = ((pre.abs() < MARGIN_COLOUR) | ((pre - 1).abs() < MARGIN_COLOUR)).any(-1) & ~vcl0
        info = {'pre': pre.numpy(), 'vis': None if t['vis_in'] is None else t['vis_in'].reshape(-1).numpy()}
        pts2l = t['light_dir'][:, None].expand(L, Ns, 3)
        if c['kernel'] == 'sg':
            nb = c['nb']
            h = F.normalize(pts2l + t['view'][None], dim=-1)
            D = torch.exp(t['lobe'].clamp(min=0) * ((h * t['normal'][None]).sum(-1, keepdim=True) - 1)).reshape(L * Ns, 1, nb)
            w = t['weights'].tile(L, 1).view(L * Ns, -1, nb)
            raw, mag = (w * D).sum(-1), (w.abs() * D).sum(-1)   # [L*Ns, 3 or 1]
            near = near | (raw.abs() < MARGIN_CANCEL * mag).any(-1)
            info['raw'] = raw.numpy()
        else:
            lh, vh, nh = (F.normalize(x, dim=-1, eps=1e-6) for x in (pts2l, t['view'][None], t['normal'][None]))
            hh = F.normalize(lh + vh, dim=-1, eps=1e-6)
            dots = torch.stack([(hh * nh).sum(-1), (hh * vh).sum(-1), (nh * vh).sum(-1).expand(L, Ns), (lh * nh).sum(-1)])
            near = near | (dots.abs() < MARGIN_DOT).any(0).reshape(-1)
            info['chi_d'] = ((hh * nh).sum(-1) > 0).reshape(-1).numpy()
    return near, info


_CASES = {}


def make_case(spec):
    """The complete case: draw_inputs + 'ambiguous' [L*Ns] bool + upstream gradients that are ZERO on the ambiguous pairs, so that
    whichever side of the step an evaluation takes there contributes nothing to any gradient.  Cached; treat as read-only."""
    key = case_id(spec) + '/%d' % spec['seed']
    if key not in _CASES:
        c = draw_inputs(spec)
        amb, info = ambiguous_pairs(c)
        keep = (~amb).to(torch.float32)[:, None]
        c['ambiguous'], c['info'] = amb, info
        c['g_rgb'] = c['g_rgb'] * keep
        if c.get('g_spec_in') is not None:
            c['g_spec_in'] = c['g_spec_in'] * keep
        _CASES[key] = c
    return _CASES[key]


_REFS = {}


def reference(spec, dtype, backward=True):
    """The oracle's formulas with autograd in ``dtype`` (torch.float64 = truth, torch.float32 on the CPU = the reference arithmetic)
    -> dict of float64 ndarrays: rgb, spec (SG), pre, and the gradients of (rgb * g_rgb).sum() + (spec * g_spec).sum():
    d_light_dir [L,3], d_normal, d_albedo [Ns,3], d_weights [Ns,nw] | d_rough [Ns,1], d_light_int (shape of the tensor; always per
    light [L,1] for 'one', whose gradient is the sum over lights), d_vis [L*Ns,1]."""
    key = (case_id(spec), spec['seed'], dtype, backward)
    if key in _REFS:
        return _REFS[key]
    c = make_case(spec)
    t = _rows(c, dtype, leaves=backward)
    if backward and c['intensity'] == 'one':   # a per-light leaf, so that the kernel's per-light gradient has a reference too
        t['light_int'] = t['light_int'].detach().expand(c['L'], 1).clone().requires_grad_(True)
    with torch.set_grad_enabled(backward):
        out = forward(c, t)
    res = {k: out[k].detach().double().numpy() for k in out}
    if backward:
        loss = (out['rgb'] * c['g_rgb'].to(dtype)).sum()
        if c.get('g_spec_in') is not None:
            loss = loss + (out['spec'] * c['g_spec_in'].to(dtype)).sum()
        loss.backward()
        names = {'light_dir': 'd_light_dir', 'normal': 'd_normal', 'albedo': 'd_albedo', 'weights': 'd_weights', 'rough': 'd_rough',
                 'light_int': 'd_light_int', 'vis_in': 'd_vis'}
        for k, name in names.items():
            if torch.is_tensor(t.get(k)) and t[k].requires_grad:
                gr = t[k].grad
                res[name] = (torch.zeros_like(t[k]) if gr is None else gr).double().numpy()
    _REFS[key] = res
    return res


def coverage(spec):
    """Shares, over the NON-ambiguous pairs of a case, of the pairs on the far side of every mask -> (ambiguous share, {name: share})."""
    c = make_case(spec)
    ok = ~c['ambiguous'].numpy()
    info, n = c['info'], max(int(ok.sum()), 1)
    sides = {'colour < 0': (info['pre'] < 0).any(-1), 'colour > 1': (info['pre'] > 1).any(-1)}
    if info['vis'] is not None:
        sides['vis < 0'], sides['vis > 1'] = info['vis'] < 0, info['vis'] > 1
    if 'raw' in info:
        sides['specular sum < 0'] = (info['raw'] < 0).any(-1)
    if 'chi_d' in info:
        sides['chi_D = 0'] = ~info['chi_d']
    return 1.0 - ok.mean(), {k: float((v & ok).sum()) / n for k, v in sides.items()}
