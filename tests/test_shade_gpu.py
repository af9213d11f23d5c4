"""The SG and GGX shading kernels (csrc/shade.hip: psn_sg_shade_fwd/_bwd, psn_mf_shade_fwd/_bwd and the light reduction both
backward passes share) against the float64 definition of tests/shade_cases.py, element by element, at two levels: the ctypes
wrappers hip.sg_shade_* / hip.mf_shade_* and ops.sg_shade / ops.mf_shade under torch.autograd.

Shapes (shade_cases.SHAPES): Ns in {1, 63, 64, 65, 130, 257} = one thread per point in 64-point workgroups with an idle-lane tail,
1 / 2 / 3 / 5 workgroups around the stride 4 of the light reduce; L in {1, 2, 3, 4, 5, 17} = SG light phases without a light
(L < 4) and a second reduce workgroup with a tail (4 L = 68 > 64).  Variants are spread over the shapes: nb 1 / 5 / 9,
specular_rgb, the light intensity as a python float / [1,1] / [L,1] / [L,3] tensor, visibility absent / detached / with a
gradient, g_spec absent / present.  tests/test_shade_cpu.py asserts that every case masks at most 10 % of its pairs as ambiguous
and has pairs on both sides of every clamp.

Tolerance: none chosen.  Per tensor, bound = 1e-5 |truth| + 1e-5 max|truth| with truth = the oracle's formulas in float64;
r_ref = the same formulas in float32 on the CPU against truth, r_hip = the kernel against truth, both in units of the bound.
The kernel may have as many elements beyond the bound as the reference arithmetic has beyond half of it, and its worst element
may be max(1, 2 max r_ref) (tests/helpers.py: a second fp32 evaluation with independent rounding differs from the first by up to
the sum of both errors).  The reference arithmetic itself, measured on the CPU over all cases: SG at most 0.27 of the bound
(d_normal: the e^10 lobe multiplies the rounding of h.n); GGX d_normal 8.7, d_light_dir 6.3, d_rough 1.2, everything else below
0.51 -- roughness 0.05 makes a2 = 6e-6, which the fp32 rounding of tan^2 = (1 - c^2) / c^2 next to the peak of D reaches.

Measured on an MI355X (gfx950), worst case over all cases, in units of the bound: r_hip (r_ref of the same case).  The two levels
agree in every figure except d_light_int, whose [1,1] form is compared as the sum over lights at the ops level.
    SG    rgb 0.073 (0.073)   spec 0.178 (0.077)   d_light_dir 0.060 (0.057)   d_light_int 0.017 (0.025) raw, 0.011 (0.007) ops
          d_normal 0.618 (0.265)   d_albedo 0.009 (0.005)   d_weights 0.091 (0.026)   d_vis 0.012 (0.012)
    GGX   rgb 0.503 (0.105)   d_light_dir 6.287 (6.298)   d_light_int 0.127 (0.210) raw, 0.283 (0.122) ops
          d_normal 8.730 (8.704)   d_albedo 0.008 (0.005)   d_rough 1.176 (1.176)   d_vis 0.485 (0.483)
Every SG tensor stays inside the plain bound; expf against torch's exp shows in spec / d_normal / d_weights (2.3 - 3.5 x the reference
arithmetic's error, still below 0.62 of the bound).  The GGX tensors beyond the bound are beyond it in the reference arithmetic by the
same amount (low-roughness peak of D).
"""
import numpy as np
import pytest
import torch

from tests import shade_cases as sc
from tests.helpers import assert_vs_truth

pytestmark = pytest.mark.gpu
RTOL = 1e-5
_WORST = {}   # (kernel, level, tensor) -> (worst r_hip, r_ref of that case, case)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _WORST:
        print('\n==== shading kernels vs float64: worst r_hip (the reference arithmetic in the same case) ====')
        for (kernel, level, name), (rh, rr, where) in sorted(_WORST.items()):
            print('%-3s %-4s %-12s r_hip %7.3f  r_ref %7.3f  (%s)' % (kernel, level, name, rh, rr, where))


def check(spec, level, name, got, keep=None, ref_name=None, reduce=None):
    """One tensor of one case against truth under the measured allowance; ``keep``: the rows compared; ``reduce``: applied to
    both references (the [1,1] intensity's gradient is the sum over lights)."""
    ref_name = ref_name or name
    t, r = sc.reference(spec, torch.float64)[ref_name], sc.reference(spec, torch.float32)[ref_name]
    if reduce is not None:
        t, r = reduce(t), reduce(r.astype(np.float32))
    got = got.detach().cpu().numpy().reshape(t.shape)
    if keep is not None:
        got, t, r = got[keep], t[keep], r[keep]
    rh, rr = assert_vs_truth('%s %s %s' % (sc.case_id(spec), level, name), got, r, t, RTOL, 'max')
    key = (spec['kernel'], level, name)
    if rh > _WORST.get(key, (-1.0,))[0]:
        _WORST[key] = (rh, rr, sc.case_id(spec))


def on_device(c, cuda):
    d = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in c.items() if k != 'info'}
    return d


def raw_intensity(d):
    """(light_int tensor or None, scalar) as ops.py hands an intensity to the ctypes wrappers."""
    li = d['light_int']
    if not torch.is_tensor(li):
        return None, float(li)
    if li.dim() == 2 and li.shape[1] == 3:
        return li.contiguous(), 0.0
    return (li.reshape(-1).expand(d['L']).contiguous() if li.numel() == 1 else li.reshape(-1).contiguous()), 0.0


def sg_raw(d, backward=True, want_vis=None):
    from psnerf_amd import hip
    li_t, li_s = raw_intensity(d)
    vis = None if d['vis_in'] is None else d['vis_in'].reshape(-1).contiguous()
    args = (d['light_dir'], d['view'], d['normal'], d['albedo'], d['weights'], d['lobe'])
    out = dict(zip(('rgb', 'spec'), hip.sg_shade_fwd(*args, li_t, li_s, vis, d['specular_rgb'])))
    if backward:
        want_vis = d['vis'] == 'grad' if want_vis is None else want_vis
        names = ('d_albedo', 'd_weights', 'd_normal', 'd_vis', 'd_light_dir', 'd_light_int')
        out.update(zip(names, hip.sg_shade_bwd(*args, li_t, li_s, vis, d['specular_rgb'], d['g_rgb'].contiguous(),
                                               d.get('g_spec_in'), want_vis)))
    return out


def mf_raw(d, backward=True, want_vis=None):
    from psnerf_amd import hip
    li_t, li_s = raw_intensity(d)
    vis = None if d['vis_in'] is None else d['vis_in'].reshape(-1).contiguous()
    args = (d['light_dir'], d['view'], d['normal'], d['albedo'], d['rough'].reshape(-1).contiguous())
    out = {'rgb': hip.mf_shade_fwd(*args, li_t, li_s, sc.F0, vis)}
    if backward:
        want_vis = d['vis'] == 'grad' if want_vis is None else want_vis
        names = ('d_albedo', 'd_rough', 'd_normal', 'd_vis', 'd_light_dir', 'd_light_int')
        out.update(zip(names, hip.mf_shade_bwd(*args, li_t, li_s, sc.F0, vis, d['g_rgb'].contiguous(), want_vis)))
    return out


def through_ops(d):
    """ops.sg_shade / ops.mf_shade under autograd -> the same dict of names as the raw level."""
    from psnerf_amd import ops
    leaf = lambda k: d[k].clone().requires_grad_(True)
    ld, n, alb = leaf('light_dir'), leaf('normal'), leaf('albedo')
    li = d['light_int'].clone().requires_grad_(True) if torch.is_tensor(d['light_int']) else d['light_int']
    vis = None if d['vis_in'] is None else d['vis_in'].clone().requires_grad_(d['vis'] == 'grad')
    if d['kernel'] == 'sg':
        mat = leaf('weights')
        rgb, spec = ops.sg_shade(ld, d['view'], n, alb, mat, d['lobe'], li, vis, d['specular_rgb'])
        out = {'rgb': rgb, 'spec': spec}
        loss = (rgb * d['g_rgb']).sum()
        if d.get('g_spec_in') is not None:   # otherwise only rgb is used downstream: backward receives g_spec = None
            loss = loss + (spec * d['g_spec_in']).sum()
    else:
        mat = leaf('rough')
        rgb = ops.mf_shade(ld, d['view'], n, alb, mat, li, vis, sc.F0)
        out = {'rgb': rgb}
        loss = (rgb * d['g_rgb']).sum()
    loss.backward()
    out.update(d_light_dir=ld.grad, d_normal=n.grad, d_albedo=alb.grad, d_light_int=li.grad if torch.is_tensor(li) else None,
               d_vis=None if vis is None else vis.grad)
    out['d_weights' if d['kernel'] == 'sg' else 'd_rough'] = mat.grad
    return out


def compare(spec, level, out):
    c = sc.make_case(spec)
    L, Ns, mf = c['L'], c['Ns'], c['kernel'] == 'mf'
    keep = ~c['ambiguous'].numpy()
    assert out['rgb'].shape == (L * Ns, 3)
    check(spec, level, 'rgb', out['rgb'], keep=keep if mf else None)   # D jumps at h.n = 0; the SG forward is continuous
    if not mf:
        assert out['spec'].shape == (L * Ns, 3 if c['specular_rgb'] else 1)
        check(spec, level, 'spec', out['spec'])
    for name in ('d_light_dir', 'd_normal', 'd_albedo', 'd_rough' if mf else 'd_weights'):
        assert out[name].shape == sc.reference(spec, torch.float64)[name].shape[:out[name].dim()]   # (raw d_rough is [Ns])
        check(spec, level, name, out[name])
    if c['intensity'] == 'float':
        assert out['d_light_int'] is None
    elif c['intensity'] == 'one' and level == 'ops':
        assert out['d_light_int'].shape == (1, 1)
        check(spec, level, 'd_light_int', out['d_light_int'], reduce=lambda x: x.sum().reshape(1, 1))
    else:
        assert out['d_light_int'].shape == ((L,) if level == 'raw' else (L, 1))
        check(spec, level, 'd_light_int', out['d_light_int'])
    if c['vis'] == 'grad':
        assert out['d_vis'].shape == ((L * Ns,) if level == 'raw' else (L * Ns, 1))
        check(spec, level, 'd_vis', out['d_vis'])
        v = c['vis_in'].reshape(-1).numpy()
        assert not out['d_vis'].detach().cpu().numpy().reshape(-1)[(v < 0) | (v > 1)].any(), 'd_vis outside [0, 1]'
    else:
        assert out['d_vis'] is None   # absent or detached: the wrapper returns none


@pytest.mark.parametrize('spec', sc.SG_CASES + sc.MF_CASES, ids=sc.case_id)
def test_raw_kernels_vs_float64(cuda, spec):
    d = on_device(sc.make_case(spec), cuda)
    compare(spec, 'raw', (sg_raw if spec['kernel'] == 'sg' else mf_raw)(d))


@pytest.mark.parametrize('spec', sc.SG_CASES + sc.MF_CASES, ids=sc.case_id)
def test_autograd_ops_vs_float64(cuda, spec):
    compare(spec, 'ops', through_ops(on_device(sc.make_case(spec), cuda)))


@pytest.mark.parametrize('spec', sc.SG_RGB_LIGHT_CASES, ids=sc.case_id)
def test_sg_rgb_lights_forward_only(cuda, spec):
    """[L,3] intensities (stage2/eval.py:200) against the per-channel reference; a gradient through them is refused."""
    from psnerf_amd import ops
    d = on_device(sc.make_case(spec), cuda)
    assert d['light_int'].shape == (d['L'], 3)
    out = sg_raw(d, backward=False)
    for level, o in (('raw', out), ('ops', dict(zip(('rgb', 'spec'), ops.sg_shade(
            d['light_dir'], d['view'], d['normal'], d['albedo'], d['weights'], d['lobe'], d['light_int'], d['vis_in'], d['specular_rgb']))))):
        for name in ('rgb', 'spec'):
            t, r = (sc.reference(spec, dt, backward=False)[name] for dt in (torch.float64, torch.float32))
            assert_vs_truth('%s %s %s' % (sc.case_id(spec), level, name), o[name].cpu().numpy(), r, t, RTOL, 'max')
    for k in ('light_dir', 'normal', 'albedo', 'weights', 'light_int'):
        a = {n: d[n] for n in ('light_dir', 'normal', 'albedo', 'weights', 'light_int')}
        a[k] = a[k].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match='forward-only'):
            ops.sg_shade(a['light_dir'], d['view'], a['normal'], a['albedo'], a['weights'], d['lobe'], a['light_int'], d['vis_in'],
                         d['specular_rgb'])


@pytest.mark.parametrize('kernel', ['sg', 'mf'])
def test_backward_is_deterministic(cuda, kernel):
    """Fixed-order reductions: two backward passes on (130, 17) agree bit for bit in every output."""
    spec = [s for s in (sc.SG_CASES if kernel == 'sg' else sc.MF_CASES) if (s['Ns'], s['L']) == (130, 17)][0]
    d = on_device(sc.make_case(spec), cuda)
    a, b = ((sg_raw if kernel == 'sg' else mf_raw)(d, want_vis=True) for _ in range(2))
    assert sorted(a) == sorted(b) and len(a) >= 7
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _known(cuda, kernel, light, view, normal, albedo, light_int, vis, g_rgb, weights=None, rough=None, nb=9):
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=cuda)
    L, Ns = len(light), len(normal)
    d = dict(kernel=kernel, L=L, Ns=Ns, light_dir=f(light), view=f(view), normal=f(normal), albedo=f(albedo),
             light_int=f(light_int).reshape(L, 1), vis_in=None if vis is None else f(vis).reshape(L * Ns, 1), vis='grad',
             g_rgb=f(g_rgb).reshape(L * Ns, 3), specular_rgb=True)
    if kernel == 'sg':
        d.update(weights=f(weights).reshape(Ns, 3 * nb), lobe=f([np.exp(i) for i in range(2, 2 + nb)]))
        return sg_raw(d)
    d['rough'] = f(rough).reshape(Ns, 1)
    return mf_raw(d)


def test_sg_known_answers(cuda):
    f32 = np.float32
    # (1) light (1,0,0) on normal (0,1,0): cos = 0 exactly, colour exactly 0, and the inclusive clamp still passes the gradient:
    #     d_albedo = g I cos vis = 0, d_light_dir = g brdf I vis n (powers of two: exact scalings of brdf = albedo + spec)
    w = np.linspace(0.1, 0.9, 27)
    for ch in range(3):
        g = np.zeros(3)
        g[ch] = 2.0
        o = _known(cuda, 'sg', [[1, 0, 0]], [[0.6, 0.8, 0]], [[0, 1, 0]], [[0.3, 0.5, 0.7]], [4.0], [0.5], [g.tolist()], weights=w)
        assert torch.equal(o['rgb'], torch.zeros_like(o['rgb'])) and float(o['spec'].min()) > 0
        brdf = (torch.tensor([0.3, 0.5, 0.7]) + o['spec'].cpu()[0])[ch]   # one fp32 addition, as the kernel forms it
        want = float(f32(2.0) * f32(brdf) * f32(4.0) * f32(0.5))
        assert o['d_light_dir'].cpu().tolist() == [[0.0, want, 0.0]]
        assert o['d_normal'].cpu().tolist() == [[want, 0.0, 0.0]]        # d cos / d n = l; the lobe path carries g I cos vis = 0
        assert not o['d_albedo'].any() and not o['d_weights'].any() and not o['d_vis'].any()
        assert o['d_light_int'].cpu().tolist() == [0.0]
    # (2) visibility exactly 0 and exactly 1 pass d_vis (the same value as at 0.5: it does not depend on vis), -0.25 and 1.25 give 0
    pt = lambda x: [x] * 5
    o = _known(cuda, 'sg', [[0.0, 0.6, 0.8]], pt([0.6, 0.8, 0]), pt([0, 1, 0]), pt([0.3, 0.5, 0.7]), [0.5], [0.0, 1.0, 0.5, -0.25, 1.25],
               pt([1.0, 1.0, 1.0]), weights=np.tile(w * 0.1, 5))
    dv = o['d_vis'].cpu()
    assert float(dv[2]) > 0 and float(dv[0]) == float(dv[2]) == float(dv[1]) and dv[3:].tolist() == [0.0, 0.0]
    assert float(o['rgb'][1].max()) < 1   # (so that the colour clamp is not what decides above)
    # (3) all-zero weights: spec == 0 and rgb == clamp(albedo I cos vis), in the kernel's operation order
    c = sc.make_case(sc.SG_CASES[6])
    d = on_device(c, cuda)
    d['weights'] = torch.zeros_like(d['weights'])
    o = sg_raw(d, backward=False)
    assert not o['spec'].any()
    l, n = c['light_dir'], c['normal']
    cos = ((l[:, None, 0] * n[None, :, 0] + l[:, None, 1] * n[None, :, 1]) + l[:, None, 2] * n[None, :, 2]).reshape(-1, 1)
    want = ((c['albedo'].tile(c['L'], 1) * c['light_int'].repeat_interleave(c['Ns'], 0)) * cos * c['vis_in'].clamp(0, 1)).clamp(0, 1)
    assert torch.equal(o['rgb'].cpu(), want)
    # (4) l = -v: h = 0 / 1e-12 = 0, D_k = exp(-lambda_k); forward only (the view from behind, so that cos > 0)
    spec = dict(sc.SG_CASES[5], seed=160)
    assert (spec['L'], spec['intensity'], spec['vis']) == (1, 'one', None)
    c2 = dict(sc.draw_inputs(spec))
    c2['view'] = -c2['light_dir'].expand(c2['Ns'], 3).contiguous()
    c2['normal'] = torch.nn.functional.normalize(c2['normal'] + 2 * c2['light_dir'], dim=-1) * 0.95
    o = sg_raw(on_device(c2, cuda), backward=False)
    t = {dt: sc.forward(c2, sc._rows(c2, dt)) for dt in (torch.float64, torch.float32)}
    lam = c2['lobe'].double().clamp(min=0)
    want = (c2['weights'].double().view(c2['Ns'], -1, spec['nb']) * torch.exp(-lam)).sum(-1).clamp(min=0)
    assert torch.allclose(t[torch.float64]['spec'], want, rtol=1e-12, atol=0) and float(want.max()) > 0
    for name in ('rgb', 'spec'):
        got = o[name].cpu().numpy()
        assert np.isfinite(got).all()
        assert_vs_truth('l = -v ' + name, got, t[torch.float32][name].numpy(), t[torch.float64][name].numpy(), RTOL, 'max')
    assert float(o['rgb'].max()) > 0


def test_mf_known_answers(cuda):
    f32 = np.float32
    # (1) cos = 0 exactly; the view from behind makes chi_D = 0, so brdf = albedo / pi: colour 0, d_albedo 0, d_light_dir = g brdf I vis n
    alb = [0.3, 0.5, 0.7]
    for ch in range(3):
        g = np.zeros(3)
        g[ch] = 2.0
        o = _known(cuda, 'mf', [[1, 0, 0]], [[0, -1, 0]], [[0, 1, 0]], [alb], [4.0], [0.5], [g.tolist()], rough=[0.5])
        assert torch.equal(o['rgb'], torch.zeros_like(o['rgb']))
        want = float(f32(2.0) * (f32(alb[ch]) / f32(np.pi)) * f32(4.0) * f32(0.5))
        assert o['d_light_dir'].cpu().tolist() == [[0.0, want, 0.0]]
        assert not o['d_albedo'].any() and not o['d_vis'].any() and not o['d_rough'].any()
        assert o['d_light_int'].cpu().tolist() == [0.0]
    # (2) visibility exactly 0 / 1 pass d_vis, -0.25 / 1.25 give 0
    pt = lambda x: [x] * 5
    o = _known(cuda, 'mf', [[0.0, 0.6, 0.8]], pt([0.6, 0.8, 0]), pt([0, 1, 0]), pt(alb), [0.5], [0.0, 1.0, 0.5, -0.25, 1.25],
               pt([1.0, 1.0, 1.0]), rough=pt(0.6))
    dv = o['d_vis'].cpu()
    assert float(dv[2]) > 0 and float(dv[0]) == float(dv[2]) == float(dv[1]) and dv[3:].tolist() == [0.0, 0.0]
    assert float(o['rgb'][1].max()) < 1
    # (3) l = -v: l^ + v^ = 0, h = 0 / 1e-6 = 0 -> D = G = 0, brdf = albedo / pi; forward only (the view from behind: cos > 0)
    spec = dict(sc.MF_CASES[5], seed=260)
    assert (spec['L'], spec['intensity'], spec['vis']) == (1, 'one', None)
    c2 = dict(sc.draw_inputs(spec))
    c2['view'] = -c2['light_dir'].expand(c2['Ns'], 3).contiguous()
    c2['normal'] = c2['normal'] + 6 * c2['light_dir']
    o = mf_raw(on_device(c2, cuda), backward=False)
    t = {dt: sc.forward(c2, sc._rows(c2, dt)) for dt in (torch.float64, torch.float32)}
    got = o['rgb'].cpu().numpy()
    assert np.allclose(t[torch.float64]['pre'].numpy(), (c2['albedo'].double() / np.pi * c2['light_int'].double()
                       * (c2['normal'].double() @ c2['light_dir'][0].double())[:, None]).numpy(), rtol=1e-12, atol=0)
    assert np.isfinite(got).all() and float(got.max()) > 0
    assert_vs_truth('l = -v rgb', got, t[torch.float32]['rgb'].numpy(), t[torch.float64]['rgb'].numpy(), RTOL, 'max')


@pytest.mark.parametrize('kernel', ['sg', 'mf'])
def test_no_points_no_launch(cuda, kernel):
    """Ns = 0: empty outputs, zero light gradients (a sum over no points), nothing launched -- at both levels."""
    spec = dict((sc.SG_CASES if kernel == 'sg' else sc.MF_CASES)[6])
    d = on_device(sc.make_case(spec), cuda)
    for k in ('view', 'normal', 'albedo', 'weights', 'rough', 'vis_in', 'g_rgb', 'g_spec_in'):
        if torch.is_tensor(d.get(k)):
            d[k] = d[k][:0].contiguous()
    d['Ns'] = 0
    for level, out in (('raw', (sg_raw if kernel == 'sg' else mf_raw)(d, want_vis=True)), ('ops', through_ops(d))):
        assert out['rgb'].shape == (0, 3) and out['d_albedo'].shape == (0, 3) and out['d_normal'].shape == (0, 3)
        assert out['d_vis'].numel() == 0
        assert out['d_light_dir'].shape == (d['L'], 3) and not out['d_light_dir'].any()
        assert out['d_light_int'].numel() == d['L'] and not out['d_light_int'].any()
