"""Cases and references for the stage-1 ray pipeline (csrc/composite.hip, csrc/sample.hip): plain data and CPU code, nothing here
touches a GPU.  tests/test_ray_cpu.py checks the cases themselves (dispatch table covered, grid caps straddled, the float32
reference inside the cap of its allowance, wrong formulas rejected); tests/test_ray_gpu.py runs the kernels on them.

Composite.  Reference = oracle.stage1.alpha_composite (rendering.py:196-197) + the white-background line rendering.py:214-216,
with autograd; float64 on the float32 inputs cast up is the truth, float32 on the CPU the reference arithmetic.  Bound per
tensor: helpers.assert_vs_truth with rtol 1e-5 and atol ATOL_UNIT (w, rgb, acc) or 'max' (d_alpha, d_rgb), both multiplied by
the case's SCALE (1 below 512 samples).

first_crossing / sample_points: the torch formulations of rendering.py:457-504 and :110-176 in the reference's op order, to be
met bit for bit.

The per-ray kernels around the root finder (psn_secant_step, psn_stage1_rays, psn_surface_points, psn_stage1_targets,
psn_shadow_points; last section): numpy definitions in the reference's op order, float32 to be met bit for bit, float64 as the
truth of the real-number outputs.
"""
import functools

import numpy as np
import torch

from tests.helpers import ATOL_UNIT

EPS = 1e-6   # rendering.py:8 = kEps of csrc/composite.hip
RTOL = 1e-5

# ---------------------------------------------------------------------------------------------------------------- dispatcher
# Constants of psn_composite_fwd / psn_composite_bwd, read from csrc/composite.hip: 4 waves per workgroup (kWavesPerBlock), the
# grid caps of the launches, rays per wave.  CAP = blocks x 4 waves x rays per wave = the rays of ONE pass of the grid-stride loop.
WAVES = 4
RAYS_PER_WAVE = {'blocked': 1, 'flat': 1, 'multi16': 4, 'multi32': 2, 'acc4': 4, 'bwd': 1}
GRID_CAP = {'blocked': 256 * 16, 'flat': 256 * 16, 'multi16': 256 * 8, 'multi32': 256 * 16, 'acc4': 256 * 32, 'bwd': 256 * 16}
CAP = {k: GRID_CAP[k] * WAVES * RAYS_PER_WAVE[k] for k in GRID_CAP}
assert CAP == {'blocked': 16384, 'flat': 16384, 'multi16': 32768, 'multi32': 32768, 'acc4': 131072, 'bwd': 16384}


def template_E(S):
    """E of launch_fwd<E> / launch_bwd<E>: ceil(S / 64) rounded up to 1, 2, 4, 8, 16."""
    e = (S + 63) // 64
    return 1 if e <= 1 else 2 if e <= 2 else 4 if e <= 4 else 8 if e <= 8 else 16


def fwd_path(rgb_none, need_weights, S, aligned):
    """The conditions of psn_composite_fwd in order -> (kernel, E, vec).  ``aligned``: alpha, rgb and weights all 16-byte
    aligned (hip.composite_fwd allocates the weights itself, so only alpha and rgb can be offset)."""
    assert 1 <= S <= 1024
    if rgb_none and not need_weights and S % 16 == 0 and S // 16 >= 4 and S <= 128 and (S // 16) % 4 == 0 and aligned:
        return ('acc4', S // 16, True)
    if not need_weights and not rgb_none and 64 < S <= 128:
        return ('flat', 2, False)
    if not rgb_none and need_weights and S % 4 == 0 and S < 128 and aligned:
        return ('multi16', 4, True) if S <= 64 else ('multi32', 4, True)
    E = template_E(S)
    return ('blocked', E, E >= 2 and S % E == 0 and aligned)


def bwd_path(S):
    return ('bwd', template_E(S), False)


# --------------------------------------------------------------------------------------------------------------------- cases
# mode: 'w' = colours + weights output, 'nw' = colours, no weights (ops.AlphaComposite, the training path), 'op' = opacity only
# (light visibility).  S per mode = the issue's dispatch table; 132 is added in mode 'w' because no S of that table reaches the
# blocked VECTOR kernel with E = 4 and a weights output (130 % 4 != 0: 130 and 129 both take the non-vector one), 128 because it
# is the one S <= 128 that is a multiple of four and still blocked (the multi-ray launch asks S < 128).
FWD_S = {
    'w': [1, 7, 63, 65, 127, 128, 129, 130, 132, 300, 512, 1000, 1024,   # blocked, E = 1 .. 16
          4, 60, 64,                                                    # several rays per wave, 16 lanes per ray
          68, 96, 124],                                                 # several rays per wave, 32 lanes per ray
    'nw': [65, 96, 127, 128,                                            # flat
           64, 129, 256],                                               # blocked
    'op': [64, 128,                                                     # four rays per wave
           16, 48, 96, 63, 256],                                        # blocked
}
BWD_S = [1, 7, 64, 65, 96, 128, 130, 300, 1024]
BWD_FORMS = ('white', 'black', 'no_d_acc', 'no_rgb')
SMALL_N = (1, 5, 37, 130)   # four-waves-per-block and rays-per-wave tails
# one n_samples per kernel for the ray counts around its cap: (mode, S, kernel)
CAP_FWD = [('nw', 96, 'flat'), ('op', 128, 'acc4'), ('op', 64, 'acc4'), ('w', 64, 'multi16'), ('w', 96, 'multi32'),
           ('w', 130, 'blocked')]
CAP_BWD_S = 96


def cap_counts(kernel):
    C = CAP[kernel]
    return (C + 1, C + 5, 2 * C + 3)


# Scale of rtol and atol for the long rays (S = 512, 1000, 1024): the smallest power of two at which the float32 reference
# arithmetic meets the cap of test_ray_cpu.py (finite, at most 2 % of the elements beyond half the bound, worst element at most
# 4 x the bound) on every tensor of every case of that S.  Measured on the CPU with the draw below (test_ray_cpu.py prints the
# figures): the factor is 2^0 = 1 at all three.  Worst element of the reference in units of the UNSCALED bound, worst case of that
# S, and the share of elements beyond half of it:
#     S =  512:  w 0.09   acc 0.09   rgb 0.09 (black) 0.31 (white)                                        0 % everywhere
#     S = 1000:  w 0.14   acc 0.13   rgb 0.13 (black) 0.32 (white)                                        0 %
#     S = 1024:  w 0.12   acc 0.12   rgb 0.11 (black) 0.30 (white)   d_alpha 0.49 (no_rgb form), d_rgb 0.07  0 %
# A product of k factors fl(1 - a + eps) carries a random walk of sqrt(k) x 1.7e-8 = 5e-7 at k = 1000, a twentieth of rtol.  What
# takes a float32 evaluation beyond the bound at these lengths is the DRIFT of that product when every factor rounds the same way;
# draw_alpha() says how the draw keeps it out (with 300 exact zeros in a row the reference is at 1.4 x the bound).
SCALE = {512: 1, 1000: 1, 1024: 1}


def scale_of(S):
    return SCALE.get(S, 1)


def _fwd(mode, N, S, mis=None):
    return dict(kind='fwd', mode=mode, N=N, S=S, mis=mis)


def _bwd(N, S, mis=None):
    return dict(kind='bwd', mode='bwd', N=N, S=S, mis=mis)


FWD_CASES = [_fwd(mode, N, S) for mode in ('w', 'nw', 'op') for S in FWD_S[mode] for N in SMALL_N]
BWD_CASES = [_bwd(N, S) for S in BWD_S for N in SMALL_N]
FWD_CAP_CASES = [_fwd(mode, N, S) for mode, S, kernel in CAP_FWD for N in cap_counts(kernel)]
BWD_CAP_CASES = [_bwd(N, CAP_BWD_S) for N in cap_counts('bwd')]
# A contiguous view that starts one float into its buffer: alpha alone, rgb alone.  One case per path; the S are those whose
# aligned path is a vector / several-rays kernel, so that the fallback is what runs (blocked non-vector although S % E == 0,
# opacity-only acc4 -> blocked, weights multi-ray -> blocked), plus the scalar-access kernels (flat, blocked E = 1, backward)
# where only the values can change.  The weights output is allocated inside hip.composite_fwd and cannot be offset through it.
MIS_N = 37
FWD_MIS_CASES = ([_fwd('w', MIS_N, S, mis) for S in (7, 64, 96, 128, 132, 512, 1024) for mis in ('alpha', 'rgb')]
                 + [_fwd('nw', MIS_N, S, mis) for S in (96, 64, 256) for mis in ('alpha', 'rgb')]
                 + [_fwd('op', MIS_N, S, 'alpha') for S in (64, 128, 96, 256)])
BWD_MIS_CASES = [_bwd(MIS_N, S, mis) for S in (96, 130) for mis in ('alpha', 'rgb')]
ALL_FWD = FWD_CASES + FWD_MIS_CASES + FWD_CAP_CASES
ALL_BWD = BWD_CASES + BWD_MIS_CASES + BWD_CAP_CASES


def case_id(c):
    return '%s-N%d-S%d%s' % (c['mode'], c['N'], c['S'], '-off_' + c['mis'] if c['mis'] else '')


def case_path(c):
    if c['kind'] == 'bwd':
        return bwd_path(c['S'])
    return fwd_path(c['mode'] == 'op', c['mode'] == 'w', c['S'], c['mis'] is None)


def is_small(c):
    return c['N'] <= max(SMALL_N)


# -------------------------------------------------------------------------------------------------------------------- inputs
ZERO_SHARE = 2.0 / 9.0


def draw_alpha(N, S, g):
    """Opacities [N, S] float32.  Per sample: U[0, 0.3] (half), exactly 0, exactly 1, 1 - 10^U[-7, -2], U[0.3, 1] (an eighth
    each).  Every second ray (1, 3, ..) is a trained profile: k samples that are 0 or below 1e-3, one in [0.05, 0.95], 1.0 to the
    end; k uniform in [0, S), the first two such rays with k = 0 and k = S - 1.  Every eighth ray (0, 8, ..) is the trained
    profile of a ray that misses the object, k = S: 0 or below 1e-3 throughout.  Without such a ray every ray of a case with
    S >= 64 is opaque, acc = 1 - T_S + eps sum T is flat to 1e-6 in every opacity and the opacity-only gradient G T - R / t is
    the difference of two O(T) terms that leaves 1e-6 T: pure rounding in any float32 evaluation, the reference's included.

    ZERO_SHARE of the samples of a transparent run are exactly 0, the others U(0, 1e-3).  float32 rounds 1 - 0 + eps DOWN by
    4.6e-8 (1e-6 = 8.39 ulps of 1) and 1 - a + eps for a in (1e-6, 1e-3) UP by 1.3e-8 on average (16.78 ulps of 0.5), the same
    way at every sample, so a run of one kind alone makes the transmittance of the float32 reference drift linearly: 1.4e-5
    after 300 exact zeros, more than rtol.  The kernels perform the same two roundings; the drift says nothing about them but
    takes the reference out of the cap that test_ray_cpu.py puts on it.  At 2/9 zeros the two drifts cancel on average."""
    kind = torch.rand(N, S, generator=g)
    v = torch.rand(N, S, generator=g)
    a = 0.3 * v
    a = torch.where((kind >= 0.5) & (kind < 0.625), torch.zeros_like(a), a)
    a = torch.where((kind >= 0.625) & (kind < 0.75), torch.ones_like(a), a)
    a = torch.where((kind >= 0.75) & (kind < 0.875), (1.0 - torch.pow(10.0, (-7.0 + 5.0 * v).double())).float(), a)
    a = torch.where(kind >= 0.875, 0.3 + 0.7 * v, a)

    def transparent(n):
        return torch.where(torch.rand(n, S, generator=g) < ZERO_SHARE, torch.zeros(n, S), 1e-3 * torch.rand(n, S, generator=g))
    rows = torch.arange(1, N, 2)
    if rows.numel():
        k = torch.randint(0, S, (rows.numel(),), generator=g)
        k[0] = 0
        if rows.numel() > 1:
            k[1] = S - 1
        s = torch.arange(S).view(1, -1)
        mid = 0.05 + 0.9 * torch.rand(rows.numel(), 1, generator=g)
        a[rows] = torch.where(s < k.view(-1, 1), transparent(rows.numel()),
                              torch.where(s == k.view(-1, 1), mid.expand(-1, S), torch.ones(1, S)))
    rows = torch.arange(0, N, 8)
    a[rows] = transparent(rows.numel())
    return a.float().contiguous()


def _seed(c):
    return (c['S'] * 1000003 + c['N'] * 7 + ('w', 'nw', 'op', 'bwd').index(c['mode'])) % (2 ** 31)


def make_inputs(c):
    """alpha [N,S], rgb [N,S,3] (None in mode 'op'), c1 [N,3], c2 [N] -- float32 CPU tensors, the same for a case with and
    without an offset."""
    g = torch.Generator().manual_seed(_seed(c))
    N, S = c['N'], c['S']
    alpha = draw_alpha(N, S, g)
    rgb = None if c['mode'] == 'op' else torch.rand(N, S, 3, generator=g)
    return dict(alpha=alpha, rgb=rgb, c1=torch.randn(N, 3, generator=g), c2=torch.randn(N, generator=g))


def offset_by_one(t, device=None):
    """A contiguous tensor equal to ``t`` whose storage starts ONE float into a fresh buffer (numel + 1 floats): 4 mod 16."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device if device is not None else t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ----------------------------------------------------------------------------------------------------------------- reference
def _np(t):
    return None if t is None else t.detach().numpy()


def forward_reference(inp, dtype):
    """{'w', 'acc', 'rgb_black', 'rgb_white'} (no colours in mode 'op') as numpy arrays of ``dtype``."""
    from oracle import stage1 as o1
    a = inp['alpha'].to(dtype)
    with torch.no_grad():
        if inp['rgb'] is None:
            w = o1.alpha_composite(a)
            return dict(w=_np(w), acc=_np(w.sum(-1)))
        w, rgb = o1.alpha_composite(a, inp['rgb'].to(dtype))
        acc = torch.sum(w, -1)
        return dict(w=_np(w), acc=_np(acc), rgb_black=_np(rgb), rgb_white=_np(rgb + (1. - acc.unsqueeze(-1))))


def backward_reference(inp, dtype, form):
    """{'d_alpha', 'd_rgb'} of sum(rgb c1) + sum(acc c2) by autograd; forms: 'white' / 'black' background, 'no_d_acc' (white,
    no gradient into acc), 'no_rgb' (the opacity-only form: only acc c2, d_rgb None)."""
    from oracle import stage1 as o1
    a = inp['alpha'].clone().to(dtype).requires_grad_(True)
    c1, c2 = inp['c1'].to(dtype), inp['c2'].to(dtype)
    if form == 'no_rgb':
        (o1.alpha_composite(a).sum(-1) * c2).sum().backward()
        return dict(d_alpha=_np(a.grad), d_rgb=None)
    c = inp['rgb'].clone().to(dtype).requires_grad_(True)
    w, rgb = o1.alpha_composite(a, c)
    acc = torch.sum(w, -1)
    if form != 'black':
        rgb = rgb + (1. - acc.unsqueeze(-1))
    loss = (rgb * c1).sum()
    if form != 'no_d_acc':
        loss = loss + (acc * c2).sum()
    loss.backward()
    return dict(d_alpha=_np(a.grad), d_rgb=_np(c.grad))


def _reference(cid, kind, mode, N, S):
    c = dict(kind=kind, mode=mode, N=N, S=S, mis=None)
    inp = make_inputs(c)
    if kind == 'fwd':
        return {dt: forward_reference(inp, dt) for dt in (torch.float64, torch.float32)}
    return {dt: {f: backward_reference(inp, dt, f) for f in BWD_FORMS} for dt in (torch.float64, torch.float32)}


_reference_small = functools.lru_cache(maxsize=None)(_reference)


def reference(c):
    """{float64: truth, float32: reference arithmetic} of a case, computed once for the small cases and shared (read only)."""
    key = (case_id(dict(c, mis=None)), c['kind'], c['mode'], c['N'], c['S'])
    return _reference_small(*key) if is_small(c) else _reference(*key)


def tensors(c, ref):
    """[(name, truth, fp32 reference, atol)] of a case: forward w / acc / rgb for both backgrounds, backward per form."""
    t, r = ref[torch.float64], ref[torch.float32]
    if c['kind'] == 'fwd':
        return [(k, t[k], r[k], ATOL_UNIT) for k in ('w', 'acc', 'rgb_black', 'rgb_white') if k in t]
    return [('%s %s' % (k, f), t[f][k], r[f][k], 'max') for f in BWD_FORMS for k in ('d_alpha', 'd_rgb') if t[f][k] is not None]


def bound(c, atol):
    """(rtol, atol) of a case's tensor."""
    s = scale_of(c['S'])
    return RTOL * s, (atol if isinstance(atol, str) else atol * s)


# ------------------------------------------------------------------------------------ an explicit float32 formulation, and wrong ones
def explicit_formulation(inp, white, variant=None, d_acc=True, dtype=torch.float32):
    """The composite and its gradient written out (what the kernels compute, in torch ops): forward w = a T, T the exclusive
    product of t = 1 - a + eps; backward G_s = g_acc + sum_ch g_ch (c_s,ch - wb), d_rgb = w g, d_alpha = G T - R / t with R the
    exclusive suffix sum of G w.  ``variant`` = None: correct; otherwise one deliberate mistake:
      'inclusive'   T includes the own sample           'no_carry'   T restarts at every 64-sample chunk
      'bg_sign'     rgb - (1 - acc)                     'bg_acc'     rgb + acc
      'channels'    d_rgb uses g rotated by one channel 'suffix_incl' R includes the own sample
      'no_eps'      eps = 0
    -> dict of numpy arrays w, acc, rgb, d_alpha, d_rgb."""
    a, c = inp['alpha'].to(dtype), inp['rgb'].to(dtype)
    c1, c2 = inp['c1'].to(dtype), inp['c2'].to(dtype)
    N, S = a.shape
    t = 1.0 - a + (0.0 if variant == 'no_eps' else EPS)
    if variant == 'no_carry':
        T = torch.cat([torch.cumprod(torch.cat([torch.ones(N, 1, dtype=dtype), ch], -1), -1)[:, :ch.shape[1]]
                       for ch in torch.split(t, 64, dim=1)], -1)
    elif variant == 'inclusive':
        T = torch.cumprod(t, -1)
    else:
        T = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=dtype), t], -1), -1)[:, :-1]
    w = a * T
    acc = w.sum(-1)
    rgb = (w.unsqueeze(-1) * c).sum(-2)
    if white:
        rgb = rgb - (1.0 - acc.unsqueeze(-1)) if variant == 'bg_sign' else rgb + acc.unsqueeze(-1) if variant == 'bg_acc' \
            else rgb + (1.0 - acc.unsqueeze(-1))
    wb = 1.0 if white else 0.0
    G = ((c - wb) * c1.unsqueeze(1)).sum(-1) + (c2.unsqueeze(1) if d_acc else 0.0)
    gw = G * w
    incl = torch.flip(torch.cumsum(torch.flip(gw, [-1]), -1), [-1])
    R = incl if variant == 'suffix_incl' else torch.cat([incl[:, 1:], torch.zeros(N, 1, dtype=dtype)], -1)
    d_alpha = G * T - R / t
    g = torch.roll(c1, 1, -1) if variant == 'channels' else c1
    d_rgb = w.unsqueeze(-1) * g.unsqueeze(1)
    return dict(w=_np(w), acc=_np(acc), rgb=_np(rgb), d_alpha=_np(d_alpha), d_rgb=_np(d_rgb))


WRONG_VARIANTS = ('inclusive', 'no_carry', 'bg_sign', 'bg_acc', 'channels', 'suffix_incl', 'no_eps')

# =============================================================================================================== first crossing
FC_M = (2, 3, 64, 65, 128, 256, 257)
FC_N = (1, 3, 4, 5, 261)   # four rays per workgroup: 1 / 3 / 4 / 5 rays and a tail after 65 workgroups
FC_TAU, FC_NEAR = 0.5, 28.0
FC_CASES = [(M, N) for M in FC_M for N in FC_N]


def _profile(M, start_free, changes, g):
    """occupancy [M]: free = U[0.05, 0.4], occupied = U[0.6, 0.95]; the state flips AFTER every sample number in ``changes``
    (a change at m = the pair (m, m + 1) has one sample on each side of tau)."""
    free = start_free
    state = torch.empty(M, dtype=torch.bool)
    for m in range(M):
        state[m] = free
        if m in changes:
            free = not free
    r = torch.rand(M, generator=g)
    return torch.where(state, 0.05 + 0.35 * r, 0.6 + 0.35 * r).float()


def crossing_profiles(M):
    """[(name, occ [M], expect)]: the constructed profiles that exist at this M, one ray each; expect = the sample number of the
    crossing that must be reported, or -1 where the mask must stay clear (what the construction says, not what any code gives)."""
    g = torch.Generator().manual_seed(4000 + M)
    tau = np.float32(FC_TAU)
    below, above = float(np.nextafter(tau, np.float32(0))), float(np.nextafter(tau, np.float32(1)))
    P = [('all free', _profile(M, True, [], g), -1), ('all occupied', _profile(M, False, [], g), -1)]
    for m in sorted({0, 1, 62, 63, 64, 65, M - 2}):
        if 0 <= m <= M - 2:
            P.append(('free->occupied at %d' % m, _profile(M, True, [m], g), m))
    if M >= 3:
        # starts inside: the first change is occupied->free, the mask and the first_free bit stay clear
        P.append(('occupied->free->occupied', _profile(M, False, [(M - 1) // 3, 2 * (M - 1) // 3], g), -1))
        # a sample exactly tau between a free and an occupied one: both products are 0, no crossing in either formulation
        for m in sorted({1, 63, 64, M - 2}):
            if 1 <= m <= M - 2:
                v = _profile(M, True, [m], g)
                v[m] = FC_TAU
                P.append(('exactly tau at %d' % m, v, -1))
    if M >= 4:
        P.append(('free->occupied->free->occupied', _profile(M, True, [(M - 1) // 4, (M - 1) // 2, 3 * (M - 1) // 4], g), (M - 1) // 4))
    if M >= 8:
        v = _profile(M, True, [2, 5], g)   # exactly tau hides the way in; the first sign change is the way out at 5
        v[2] = FC_TAU
        P.append(('exactly tau at 2, occupied->free at 5', v, -1))
    if M >= 66:
        P.append(('changes at 0 and 64 (both lane 0)', _profile(M, True, [0, 64], g), 0))
        P.append(('changes at 63 and 64 (lane 63, then lane 0)', _profile(M, True, [63, 64], g), 63))
        m2 = min(M - 2, 128)
        P.append(('changes at 64 and %d' % m2, _profile(M, True, [64, m2], g), 64))
        P.append(('changes at 70 and 71', _profile(M, True, [70, 71], g), 70))
    # one ulp either side of tau
    for m in sorted({0, 63, M - 2}):
        if 0 <= m <= M - 2:
            v = _profile(M, True, [m], g)
            v[m], v[m + 1] = below, above
            P.append(('one ulp below / above tau at %d' % m, v, m))
    P.append(('every sample one ulp below tau', torch.full((M,), below), -1))
    v = torch.full((M,), below)
    v[M - 1] = above
    P.append(('one ulp below tau, last sample one ulp above', v, M - 2))
    v = torch.full((M,), above)
    v[0] = below
    P.append(('first sample one ulp below tau, then one ulp above', v, 0))
    return P


def crossing_case(M, N):
    """occ [N, M], far [N] in [33, 34], (u, 1 - u) tables and the profile names.  N = 261 holds every profile of this M (cycled
    with fresh far values); a smaller N takes a window of the list that starts at a different profile for every (M, N)."""
    P = crossing_profiles(M)
    assert len(P) <= max(FC_N)
    start = 0 if N >= len(P) else (7 * N + M) % len(P)
    pick = [(start + i) % len(P) for i in range(N)]
    g = torch.Generator().manual_seed(M * 1000 + N)
    u = torch.linspace(0.0, 1.0, steps=M)
    return dict(occ=torch.stack([P[i][1] for i in pick]).contiguous(), far=33.0 + torch.rand(N, generator=g), u=u, omu=1.0 - u,
                names=[P[i][0] for i in pick], expect=[P[i][2] for i in pick])


def first_crossing_reference(val, u, omu, near, far):
    """The tensor formulation of rendering.py:457-504 on val [N, M] = occupancy - tau (any device): -> (mask [N] bool,
    first_free [N] bool, the four bracket rows d_low, d_high, f_low, f_high [N], meaningful where mask is set)."""
    n, M = val.shape
    sgn = torch.cat([torch.sign(val[:, :-1] * val[:, 1:]), torch.ones(n, 1, device=val.device)], dim=-1)
    cost = sgn * torch.arange(M, 0, -1, device=val.device).float()
    values, idx = torch.min(cost, -1)
    gat = lambda i: torch.gather(val, 1, i.unsqueeze(-1)).squeeze(-1)
    first_free = val[:, 0] < 0
    mask = (values < 0) & (gat(idx) < 0) & first_free
    idx2 = torch.clamp(idx + 1, max=M - 1)
    dep = lambda i: (near * omu[i] + far.reshape(-1) * u[i]).reshape(-1)
    return mask, first_free, (dep(idx), dep(idx2), gat(idx), gat(idx2))


# ================================================================================================================ sample points
SP_SEGMENTS = ((64, 0), (32, 64), (3, 2), (1, 1))   # (c0, c1): c1 = 0 -> one inner segment of c0; else c0 outer + c1 inner samples
SP_N = (1, 5, 257)
SP_NEAR, SP_DELTA = 28.0, 0.35
SP_CASES = [(c0, c1, N, noise) for c0, c1 in SP_SEGMENTS for N in SP_N for noise in (False, True)]
SP_FORCED = 24   # the first rays of a case get the forced depths below, in rotation


def sample_case(c0, c1, N, noise):
    """Rays with surface depths that force the reference's sort to reorder, in rotation over the first SP_FORCED rays:
       dist - delta > far      dnp > dfp = far: the inner interval DESCENDS (non-monotone by construction when c1 >= 2)
       dist <= near + delta    the outer interval collapses to near (near (1 - u) + near u may wobble by an ulp)
       dist within delta of far   dfp clamps to far
    The ``mixed`` flags keep the forced rays as hit rays."""
    g = torch.Generator().manual_seed(c0 * 10007 + c1 * 101 + N * 3 + int(noise))
    S = c0 + c1
    cam = torch.randn(N, 3, generator=g)
    rays = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    far = 33.0 + torch.rand(N, generator=g)
    dist = 29.0 + 3.0 * torch.rand(N, generator=g)
    r = torch.rand(N, generator=g)
    for i in range(min(N, SP_FORCED)):
        k = i % 3 if N > 8 else 0   # (a case of fewer than 8 rays: every ray of the first kind)
        if k == 0:
            dist[i] = far[i] + SP_DELTA + 0.05 + 0.5 * r[i]
        elif k == 1:
            dist[i] = SP_NEAR + SP_DELTA * r[i]
        else:
            dist[i] = far[i] - SP_DELTA * r[i]
    mixed = torch.rand(N, generator=g) < 0.6
    mixed[:min(N, SP_FORCED)] = True
    if N > 1:
        mixed[-1] = False
    return dict(cam=cam, rays=rays, far=far, dist=dist, S=S, noise=torch.rand(N, S, generator=g) if noise else None,
                flags=dict(mixed=mixed, all_hit=torch.ones(N, dtype=torch.bool), all_miss=torch.zeros(N, dtype=torch.bool)))


def lin(n, device=None):
    """(linspace(0, 1, n), 1 - it), built on the CPU so that both sides read the same table."""
    u = torch.linspace(0.0, 1.0, steps=n)
    return (u.to(device), (1.0 - u).to(device)) if device is not None else (u, 1.0 - u)


def jitter(d, nz):
    """rendering.py:133-141: stratified jitter between the mid-points of neighbouring depths."""
    mid = 0.5 * (d[:, 1:] + d[:, :-1])
    hi = torch.cat([mid, d[:, -1:]], dim=-1)
    lo = torch.cat([d[:, :1], mid], dim=-1)
    return lo + (hi - lo) * nz


def hit_depths(dist, far, near, delta, steps, steps_out, u_in, u_out=None, presort=False):
    """rendering.py:110-129: [n, steps_out + steps] depths of hit rays, sorted when there is an outer segment (``presort``: the
    concatenation before the sort)."""
    dnp, dfp = dist - delta, dist + delta
    dnp = torch.where(dnp < near, torch.full_like(dnp, near), dnp)
    dfp = torch.where(dfp > far, far, dfp)
    u = u_in.view(1, -1)
    d1 = dnp.view(-1, 1) * (1.0 - u) + dfp.view(-1, 1) * u
    if steps_out:
        uo = u_out.view(1, -1)
        d_out = near * (1.0 - uo) + dnp.view(-1, 1) * uo
        d1 = torch.cat([d_out, d1], dim=-1)
        if not presort:
            d1, _ = torch.sort(d1, dim=-1)
    return d1


def sample_points_reference(cam, rays, far, dist, hit_idx, miss_idx, near, delta, steps, steps_out, u_all, u_in, u_out, nz_m, nz_h):
    """The torch formulation of rendering.py:110-176 (any device): out [N, steps_out + steps, 3] with the free-space profile on
    rows miss_idx and the hit profile on rows hit_idx; u_* = linspace(0, 1, .) tables, nz_* = jitter noise or None."""
    N, S = cam.shape[0], steps + steps_out
    d2 = near * (1.0 - u_all.view(1, -1)) + far[miss_idx].view(-1, 1) * u_all.view(1, -1)
    if nz_m is not None:
        d2 = jitter(d2, nz_m)
    ref = torch.zeros(N, S, 3, device=cam.device)
    ref[miss_idx] = cam[miss_idx].unsqueeze(-2) + rays[miss_idx].unsqueeze(-2) * d2.unsqueeze(-1)
    d1 = hit_depths(dist[hit_idx], far[hit_idx], near, delta, steps, steps_out, u_in, u_out)
    if nz_h is not None:
        d1 = jitter(d1, nz_h)
    ref[hit_idx] = cam[hit_idx].unsqueeze(-2) + rays[hit_idx].unsqueeze(-2) * d1.unsqueeze(-1)
    return ref


def sample_reference(case, c0, c1, flags):
    """CPU reference of one case under one flag set."""
    hit_idx, miss_idx = flags.nonzero(as_tuple=True)[0], (~flags).nonzero(as_tuple=True)[0]
    steps, steps_out = (c1, c0) if c1 else (c0, 0)
    nz = case['noise']
    return sample_points_reference(case['cam'], case['rays'], case['far'], case['dist'], hit_idx, miss_idx, SP_NEAR, SP_DELTA, steps,
                                   steps_out, lin(case['S'])[0], lin(steps)[0], lin(steps_out)[0] if steps_out else None,
                                   None if nz is None else nz[miss_idx], None if nz is None else nz[hit_idx])


def non_monotone_rays(case, c0, c1):
    """Number of rays (all taken as hit rays) whose concatenated outer + inner depths are not non-decreasing before the sort."""
    d = hit_depths(case['dist'], case['far'], SP_NEAR, SP_DELTA, c1, c0, lin(c1)[0], lin(c0)[0], presort=True)
    return int((d[:, 1:] < d[:, :-1]).any(-1).sum())


# ======================================================================================= the per-ray kernels around the root finder
# psn_secant_step, psn_shadow_points (csrc/sample.hip), psn_stage1_rays, psn_surface_points, psn_stage1_targets (csrc/small.hip):
# numpy transcriptions of the reference lines those files cite, every operation rounded in ``dtype`` (float32: to be met bit for
# bit; float64 on the float32 inputs cast up: the truth of the real-number outputs, helpers.assert_vs_truth with RTOL).
PR_N = (1, 255, 256, 257)    # one thread per ray, 256 per workgroup; n = 0 launches nothing


def _f32(*xs):
    return [np.ascontiguousarray(x, dtype=np.float32) for x in xs]


# ---- psn_secant_step (rendering.py:525-555)
def secant_case(n, tau):
    """Brackets d_low < d_high, f_low < 0 < f_high, rays, and the occupancies of three update steps.  From 8 rays on: ray 2 meets
    occ == tau exactly in every step (f_mid = 0 is not < 0: the HIGH end moves), ray 3 has d_low == d_high, ray 4 f_low == f_high (a
    division by zero: inf, then inf or NaN), ray 5 the benign (0, 1, -1, 1) of a miss."""
    g = torch.Generator().manual_seed(7000 + n)
    r = lambda *s: torch.rand(*s, generator=g)
    d_low = 0.5 + 0.5 * r(n)
    st = dict(d_low=d_low, d_high=d_low + 0.05 + 0.25 * r(n), f_low=-0.01 - 0.49 * r(n), f_high=0.01 + 0.49 * r(n))
    occ = r(3, n)
    if n >= 8:
        occ[:, 2] = float(np.float32(tau))
        st['d_high'][3] = st['d_low'][3]
        st['f_high'][4] = st['f_low'][4]
        for k, v in zip(('d_low', 'd_high', 'f_low', 'f_high'), (0.0, 1.0, -1.0, 1.0)):
            st[k][5] = v
    origin = torch.randn(n, 3, generator=g)
    direction = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    out = {k: v.numpy().copy() for k, v in st.items()}
    out.update(occ=occ.numpy().copy(), origin=origin.numpy().copy(), direction=direction.numpy().copy(), tau=tau, n=n)
    return out


def secant_step_definition(st, occ, tau, d_pred, origin, direction, dtype=np.float32):
    """One step on the state st = dict(d_low, d_high, f_low, f_high) -> (new state, d_pred, p_mid); occ None: the initial step."""
    T = lambda x: np.asarray(x, dtype=dtype)
    dl, dh, fl, fh = (T(st[k]) for k in ('d_low', 'd_high', 'f_low', 'f_high'))
    if occ is not None:
        fm = T(occ) - T(np.float32(tau))
        low = fm < 0
        dp = T(d_pred)
        dl, fl, dh, fh = np.where(low, dp, dl), np.where(low, fm, fl), np.where(low, dh, dp), np.where(low, fh, fm)
    with np.errstate(divide='ignore', invalid='ignore'):
        new = (-fl) * (dh - dl) / (fh - fl) + dl
        p = T(origin) + new[:, None] * T(direction)
    return dict(d_low=dl, d_high=dh, f_low=fl, f_high=fh), new, p


# ---- psn_stage1_rays (common.py:205-226, rendering.py:576-596)
RAY_SCENES = ('outside', 'inside', 'behind')
RAY_UNDER_MIN = 1e-4   # rays with |under| below it are left out of the random set (far = sqrt(under) - b is ill-conditioned there)


def rays_case(n, scene):
    """(pix [n,2], K [4,4], W [4,4], radius): fx != fy; 'outside' = the camera 1.5 units out looking at a sphere of radius 0.45 that
    about half the pixels miss (under <= 0: far = 0), 'inside' = the camera inside the sphere (every ray leaves it), 'behind' = the
    sphere behind the camera (under > 0 but sqrt(under) - b < 0: clamped to 0)."""
    g = torch.Generator().manual_seed(7100 + 10 * n + RAY_SCENES.index(scene))
    h, w = 48, 64
    K = torch.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 70.0, 66.0, 31.5, 23.25
    R = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    W = torch.eye(4)
    W[:3, :3] = R
    off = torch.tensor([0.03, -0.02, 0.05])
    W[:3, 3] = {'outside': -R[:, 2] * 1.5 + off, 'inside': R[:, 0] * 0.2 + off, 'behind': R[:, 2] * 1.5 + off}[scene]
    radius = {'outside': 0.45, 'inside': 0.8, 'behind': 0.45}[scene]
    pix = torch.stack([torch.rand(4 * n + 64, generator=g) * w, torch.rand(4 * n + 64, generator=g) * h], -1)
    pix[::3] = torch.floor(pix[::3])
    K_, W_ = K.numpy().copy(), W.numpy().copy()
    under = stage1_rays_definition(pix.numpy(), K_, W_, radius, np.float64)[3]
    keep = np.abs(under) >= RAY_UNDER_MIN
    pix = pix.numpy()[keep][:n].copy()
    assert pix.shape[0] == n
    return pix, K_, W_, radius


def stage1_rays_definition(pix, K, W, radius, dtype=np.float32, wrong=None):
    """-> (cam [n,3], rays [n,3], far [n], under [n]); K [3|4, 3|4]; radius^2 is the float32 the library is handed.
    wrong='fy': the y axis over fy (the reference divides BOTH axes by fx, common.py:220)."""
    T = lambda x: np.asarray(x, dtype=dtype)
    pix, K, W = T(pix), T(K), T(W)
    r2 = T(np.float32(float(radius ** 2)))
    fx, cx, cy = K[0, 0], K[0, 2], K[1, 2]
    qx, qy = (pix[:, 0] - cx) / fx, (pix[:, 1] - cy) / (K[1, 1] if wrong == 'fy' else fx)
    d = np.stack([qx * W[r, 0] + qy * W[r, 1] + W[r, 2] for r in range(3)], -1)
    c = np.broadcast_to(W[:3, 3], d.shape)
    nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    d = d / nrm[:, None]
    b = d[:, 0] * c[:, 0] + d[:, 1] * c[:, 1] + d[:, 2] * c[:, 2]
    cn = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    under = b * b - (cn * cn - r2)
    with np.errstate(invalid='ignore'):
        far = np.where(under > 0, np.maximum(np.sqrt(np.where(under > 0, under, 0)) - b, 0), 0).astype(dtype)
    return np.ascontiguousarray(c), d, far, under


# explicit inputs for the sign of ``under`` (identity rotation, the pixel at the principal point: the ray is (0, 0, 1)):
# (camera, radius^2 as float32, far).  b = 0 and |cam|^2 = 1: under = radius^2 - 1 exactly.
RAY_UNDER_EXPLICIT = (
    ((1.0, 0.0, 0.0), 1.0, 0.0),                                                  # under == 0: not > 0, the ray misses
    ((1.0, 0.0, 0.0), float(np.nextafter(np.float32(1), np.float32(2))), None),   # under = one ulp: far = its root
    ((1.0, 0.0, 0.0), float(np.nextafter(np.float32(1), np.float32(0))), 0.0),    # under = -half an ulp
    ((0.0, 0.0, -2.0), 1.0, 3.0),                                                  # b = -2, under = 1: far = 1 + 2
    ((0.0, 0.0, 2.0), 1.0, 0.0),                                                   # b = +2, under = 1: 1 - 2 < 0, clamped
)


# ---- psn_surface_points (rendering.py:516-522, 84-108)
def surface_case(n):
    """flags {0,1,2,3} x d_pred {finite, 0, +inf, NaN} in the first 16 rays (n = 1: flags 3 on a finite depth), random behind them."""
    g = torch.Generator().manual_seed(7200 + n)
    d = (torch.rand(n, generator=g) * 3).numpy()
    fl = torch.randint(0, 4, (n,), generator=g, dtype=torch.int32).numpy()
    table = [(f, v) for f in range(4) for v in (0.75, 0.0, np.inf, np.nan)]
    if n == 1:
        fl[0] = 3
    for i, (f, v) in enumerate(table[:n if n >= 16 else 0]):
        fl[i], d[i] = f, v
    cam = torch.randn(n, 3, generator=g).numpy()
    rays = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).numpy()
    return _f32(d)[0], fl.astype(np.int32), cam, rays


def surface_points_definition(d_pred, flags, cam, rays):
    """-> (d_i, dists, obj_mask, points) in float32."""
    d = np.where(flags & 1, d_pred, np.float32(np.inf)).astype(np.float32)     # rendering.py:519-521
    d = np.where(flags & 2, d, np.float32(0)).astype(np.float32)               # :522
    zero = d == 0
    ok = np.isfinite(d)
    dists = np.where(zero, 0, np.where(ok, d, 1)).astype(np.float32)
    return d, dists, ok & ~zero, (cam + rays * dists[:, None]).astype(np.float32)


# ---- psn_stage1_targets (common.py:172-202, training.py:166-191)
TG_SIZES = ((1, 1), (1, 7), (6, 8), (48, 64))
TG_ANGLE = 70.0


def nearest_index(pix, h, w, wrong=None):
    """grid_sample(nearest, align_corners=True, zeros padding) at x = 2 px / w - 1 -> (iy, ix, inside) in float32 op order.
    wrong='floor': floor(x + 0.5) in place of the half-to-even rint."""
    one, two = np.float32(1), np.float32(2)
    px, py = _f32(pix[:, 0], pix[:, 1])
    x, y = two * px * (one / np.float32(w)) - one, two * py * (one / np.float32(h)) - one
    fx, fy = ((x + one) / two) * np.float32(w - 1), ((y + one) / two) * np.float32(h - 1)
    rnd = (lambda v: np.floor(v + np.float32(0.5))) if wrong == 'floor' else np.rint
    rx, ry = rnd(fx), rnd(fy)
    inside = (rx >= 0) & (rx <= w - 1) & (ry >= 0) & (ry <= h - 1)
    return np.where(inside, ry, 0).astype(np.int64), np.where(inside, rx, 0).astype(np.int64), inside, fx, fy


def targets_case(h, w, n):
    """Images and pixel positions: every integer pixel (cycled), x = -1 (outside from 3 columns on: zeros), x = w and y = h (with
    align_corners=True they are x = 1: exactly the LAST pixel, inside; pixel position px reads column rint(px (w - 1) / w)), x = w + 1, y = h + 1 and (w + 5, -3) (outside), fractional
    positions, the exact ties (w / 2, .) and (., h / 2) of even sizes (fx = (w - 1) / 2: half to even), and two pixels whose normal has n2 ==
    cos(TG_ANGLE) exactly (kept) and one ulp below (dropped)."""
    g = torch.Generator().manual_seed(7300 + 100 * h + w + n)
    img = torch.rand(3, h, w, generator=g).numpy()
    mask, valid, nmask = ((torch.rand(h, w, generator=g) > t).float().numpy() for t in (0.4, 0.1, 0.3))
    normal = torch.nn.functional.normalize(torch.randn(3, h, w, generator=g), dim=0).numpy()
    cos_t = np.float32(np.cos(np.deg2rad(TG_ANGLE)))
    # pixel (0, 0), read at (0, 0), and -- unless it is the same one -- pixel (h - 1, w - 1), read at (w, h)
    nmask[0, 0] = nmask[h - 1, w - 1] = 1.0
    if (h, w) != (1, 1):
        normal[2, h - 1, w - 1] = np.nextafter(cos_t, np.float32(0))
    normal[2, 0, 0] = cos_t
    world = np.eye(4, dtype=np.float32)
    world[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0].numpy()
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    grid = np.stack([xs.reshape(-1), ys.reshape(-1)], -1).astype(np.float32)
    special = np.array([[0, 0], [w, h], [-1, 0], [w, 0], [0, h], [w + 5, -3], [w / 2, 0], [0, h / 2], [w / 2, h / 2],
                        [0.4, 0.6], [w - 1.4, h - 1.5], [w * 0.37, h * 0.61], [w + 1, 0], [0, h + 1]], dtype=np.float32)
    frac = (torch.rand(n, 2, generator=g) * torch.tensor([w + 1.0, h + 1.0]) - 0.5).numpy()
    pix = np.concatenate([special, grid, frac])[:n] if n > 1 else special[8:9]
    if pix.shape[0] < n:
        pix = np.concatenate([pix, grid[np.arange(n - pix.shape[0]) % grid.shape[0]]])
    return dict(img=img, mask=mask, valid=valid, nmask=nmask, normal=_f32(normal)[0], world=world, pix=_f32(pix)[0], cos_t=float(cos_t), h=h, w=w)


def targets_definition(c, mask=True, valid=True, nmask=True, want_normal=False, use_angle=False, wrong=None):
    """-> (rgb [n,3], mask_gt [n] float, mask_valid [n] bool, norm_mask [n] bool or None, normal_gt [n,3] or None)."""
    iy, ix, inside, _, _ = nearest_index(c['pix'], c['h'], c['w'], wrong)
    take = lambda im: np.where(inside, im[..., iy, ix], np.float32(0)).astype(np.float32)
    n = c['pix'].shape[0]
    rgb = take(c['img']).T.copy()
    mask_gt = (take(c['mask']) != 0).astype(np.float32) if mask else np.ones(n, dtype=np.float32)
    mask_valid = (take(c['valid']) != 0) if valid else np.ones(n, dtype=bool)
    nm = (take(c['nmask']) != 0) if nmask else None
    ngt = None
    if want_normal:
        nv = take(c['normal'])                                  # [3, n]
        if use_angle and nm is not None:
            nm = nm & ~(nv[2] < np.float32(c['cos_t']))          # training.py:189-190: on the unrotated normal
        Wm = c['world']
        sgn = _f32([1, -1, -1])[0]
        ngt = np.stack([nv[0] * (Wm[r, 0] * sgn[0]) + nv[1] * (Wm[r, 1] * sgn[1]) + nv[2] * (Wm[r, 2] * sgn[2]) for r in range(3)], -1)
        ngt = ngt.astype(np.float32)
    return rgb, mask_gt, mask_valid, nm, ngt


# ---- psn_shadow_points (rendering.py:378-408)
# (n_surf, n_lights, n_steps, lnear, box, kind): totals 1, 105, 666 and 600 (no multiple of 64 or 256), 1027 (five workgroups)
SH_CASES = ((1, 1, 1, 0.0, 0.55, 'random'), (7, 3, 5, 0.05, 0.55, 'random'), (37, 2, 9, 0.05, 0.55, 'random'), (50, 3, 4, 0.0, 0.55, 'edge'),
            (79, 1, 13, 0.05, 0.55, 'random'), (37, 2, 9, 0.05, 10.0, 'all'), (37, 2, 9, 0.05, 0.001, 'none'),
            (0, 3, 5, 0.05, 0.55, 'random'), (7, 0, 5, 0.05, 0.55, 'random'))
SH_LFAR = 1.2


def shadow_case(ns, nl, S, lnear, box, kind):
    g = torch.Generator().manual_seed(7400 + 1000 * ns + 10 * nl + S)
    surf = (torch.rand(ns, 3, generator=g) * 1.2 - 0.6).numpy()
    if kind == 'none':
        surf = surf + np.float32(2.0)
    if kind == 'edge':
        # step 0 of a ray with lnear = 0 is the surface point itself (d = 0 * 1 + lfar * 0): a coordinate exactly +-box is inside, one
        # ulp beyond it outside
        b = np.float32(box)
        up, dn = np.nextafter(b, np.float32(2)), np.nextafter(-b, np.float32(-2))
        for i, (axis, v) in enumerate(((0, b), (1, -b), (2, b), (0, up), (1, dn), (2, up), (0, -b), (2, dn))):
            surf[i] = 0.1
            surf[i, axis] = v
    ldir = torch.nn.functional.normalize(torch.randn(nl, 3, generator=g), dim=-1).numpy()
    u = torch.linspace(0.0, 1.0, steps=S).numpy()
    return _f32(surf, ldir, u, np.float32(1) - u)


def shadow_points_definition(surf, ldir, u, omu, lnear, lfar, box, strict=False):
    """-> (rows int64 [k] ascending, pts [k,3]): the dense rows (l ns + s) S + m whose point lies in the closed cube, and the points.
    strict: the wrong form with < in place of <=."""
    ns, nl, S = surf.shape[0], ldir.shape[0], u.shape[0]
    d = (np.float32(lnear) * omu + np.float32(lfar) * u).astype(np.float32)
    p = (surf[None, :, None, :] + (ldir[:, None, None, :] * d[None, None, :, None]).astype(np.float32)).astype(np.float32).reshape(-1, 3)
    b = np.float32(box)
    inside = ((p < b) & (p > -b)).all(-1) if strict else ((p <= b) & (p >= -b)).all(-1)
    rows = np.flatnonzero(inside).astype(np.int64)
    return rows, p[rows]
