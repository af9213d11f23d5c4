"""Inputs, case tables and the definitions for the direct tests of the kernels that produce the training loss and apply the update:
the stage-2 losses (csrc/loss.hip: stage2_loss_fwd / final / bwd), the stage-1 losses and surface normals (csrc/loss1.hip),
adam_flat_kernel (csrc/small.hip) and row_adam_kernel (csrc/loss.hip).  Every definition is plain torch, written once and evaluated in
float64 ("truth") and in float32 on the CPU ("the reference arithmetic") from the same float32 inputs; autograd differentiates.
Plain data and reference code: nothing here touches a GPU.  References are cached per case: treat them as read-only.

The case tables follow the LAUNCH code, not a workload: one case per path a launch can take (light chunks, block caps and grid-stride
loops, the slices of the final reduction, host / device counts, vector / scalar / tail branches, several launches per call).

Conditioning, asserted per case by tests/test_loss_cpu.py:
  * L1 / sign terms: prediction and target are bit-equal (a tie: gradient exactly 0) or at least MIN_GAP = 1e-3 apart;
  * surface normals: |g| is exactly 0 or at least 0.05, |n - n_neighbour| exactly 0 or at least 1e-2 (d_diff / diff amplifies the
    float32 rounding of the difference in any implementation below that);
  * at most KINK_CAP = 3 % of a case's elements sit at a kink (ties, zero rows, acc exactly 0 or 1);
  * the float32 definition stays inside the plain bound 1e-5 |truth| + 1e-5 max|truth| on every tensor (r_ref <= 1)."""
import numpy as np
import torch
import torch.nn.functional as F

RTOL = 1e-5         # tensors: bound = RTOL |truth| + RTOL max|truth| (tests/test_engines_gpu.py)
TERM_RTOL = 2e-6    # scalar loss terms and the total (the figure test_fused_losses_match_modules holds them to)
KINK_CAP = 0.03
MIN_GAP = 1e-3
G_UP = 0.37         # upstream gradient of the total, not 1


def _f64(t):
    return t.detach().double().cpu().numpy()


def _leaf(t, dtype):
    return None if t is None else t.detach().to(dtype).clone().requires_grad_(True)


def _grad(t):
    return _f64(torch.zeros_like(t) if t.grad is None else t.grad)


def _delta(g, shape):
    """Offsets of magnitude 2e-3 .. 0.3, either sign."""
    return (2e-3 + 0.3 * torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _apart(g, shape, lo=0.0, hi=1.0):
    """(prediction, target): the target uniform in [lo, hi], the prediction 2e-3 .. 0.3 away from it on either side."""
    t = lo + (hi - lo) * torch.rand(shape, generator=g)
    return t + _delta(g, shape), t


def _tie(a, b):
    """Every 101st element of ``a`` (from element 100 on) is set to its target bit for bit.  -> the bool mask of the ties."""
    k = (torch.arange(a.numel()) % 101 == 100).view(a.shape)
    a[k] = b[k]
    return k


def gap_ok(a, b):
    """Bit-equal or at least MIN_GAP apart (elements that hold NaN are not judged: nothing reads them)."""
    d = (a.double() - b.double()).abs()
    return bool((torch.isnan(d) | (d == 0) | (d >= MIN_GAP)).all())


# --------------------------------------------------------------------------- stage-2 losses
def stage2_loss(rgb, rgb_gt, alb, alb_j, wgt, wgt_j, vis, vis_gt, nrm, nrm_gt, nrm_j, mask_a, mask_b, l2, inv_denom, weight, count_dev=None):
    """oracle.stage2.MainLoss + NormalLoss with the argument list of hip.stage2_loss_fwd: rgb [L,N,3], alb [N,3], wgt [N,nb], vis
    [V,N,3] (channel 0 against vis_gt [V,N]), nrm [N,3]; absent terms are None.  Only pixels of mask_a & mask_b are READ.  term_i =
    sum_i inv_denom_i, divided by count_dev where that is given (every term 0 for a count <= 0).  -> (terms [6], weighted total)."""
    m = mask_a & mask_b
    img = (lambda d: d * d) if l2 else torch.abs
    ref = next(t for t in (rgb, alb, wgt, vis, nrm) if t is not None)
    s = [ref.new_zeros(())] * 6
    if rgb is not None:
        s[0] = img(rgb[:, m] - rgb_gt[:, m]).sum()
    if alb is not None:
        s[1] = (alb[m] - alb_j[m]).abs().sum()
    if wgt is not None:
        s[2] = (wgt[m] - wgt_j[m]).abs().sum()
    if vis is not None:
        s[3] = img(vis[:, m, 0] - vis_gt[:, m]).sum()
    if nrm is not None:
        s[4] = ((nrm[m] - F.normalize(nrm_gt[m], dim=-1)) ** 2).sum()
        if nrm_j is not None:
            s[5] = (nrm[m] - nrm_j[m]).abs().sum()
    scale = 1.0
    if count_dev is not None:
        scale = 1.0 / float(count_dev) if float(count_dev) > 0 else 0.0
    terms = torch.stack([s[i] * inv_denom[i] * scale for i in range(6)])
    return terms, sum(weight[i] * terms[i] for i in range(6))


S2_WEIGHT = (1.0, 0.05, 0.01, 0.7, 0.9, 0.03)
S2_FLOATS = ('rgb', 'rgb_gt', 'alb', 'alb_j', 'wgt', 'wgt_j', 'vis', 'vis_gt', 'nrm', 'nrm_gt', 'nrm_j')
S2_LEAVES = ('rgb', 'alb', 'alb_j', 'wgt', 'wgt_j', 'vis', 'nrm', 'nrm_j')
S2_PAIRS = (('rgb', 'rgb_gt'), ('alb', 'alb_j'), ('wgt', 'wgt_j'), ('vis0', 'vis_gt'), ('nrm', 'nrm_j'))   # the L1 / sign pairs


def _s2(id, N, L, **kw):
    """absent: terms handed in as None; masks: 'half' (each mask 70 % true), 'all', 'a_false' (mask_a all false: an empty mask);
    count: 'host' (folded into inv_denom), 'dev' (the same count as count_dev), 'dev2' (twice the local count, as under data
    parallelism), 'dev0' (count_dev = 0); poison: every float input holds NaN at the masked-out pixels."""
    d = dict(id=id, N=N, L=L, nb=9, V=3, l2=0, absent=(), masks='half', count='host', poison=False)
    d.update(kw)
    return d


# forward: min(ceil(N / 256), 256) x (8 if L >= 16 else 1) blocks, one partial each; backward: min(ceil(N / 256), 1024) x the same
S2_CASES = (
    # light chunking at N = 257 (2 x 8 = 16 partials: fewer than the 32 slices of the final reduction): one chunk | one chunk | 8 full
    # chunks | lc = 3: chunk 5 holds two lights, 6 and 7 none | lc = 3, the last chunk partial | the shipped maximum
    [_s2('L%d' % L, 257, L) for L in (1, 15, 16, 17, 23, 96)]
    # pixel coverage: one thread | a partial block | exactly one block | (257 above: two blocks) | exactly the 256 blocks of the forward
    # cap | the forward grid-stride loop | the same with 8 chunks = 2048 partials: every slice of the final reduction full | the backward
    # grid-stride loop (more than 1024 blocks of pixels)
    + [_s2('N%d-L2' % N, N, 2) for N in (1, 255, 256)]
    + [_s2('N65536-L1', 65536, 1), _s2('N65793-L1', 65793, 1), _s2('N65793-L16', 65793, 16), _s2('N262444-L1', 262444, 1)]
    # terms
    + [_s2('all-terms', 257, 3)]
    + [_s2('no-' + k, 257, 3, absent=(k,)) for k in ('alb', 'wgt', 'vis', 'nrm', 'nrm_j')]
    + [_s2('rgb-alone', 257, 3, absent=('alb', 'wgt', 'vis', 'nrm', 'nrm_j')), _s2('nb1', 257, 3, nb=1), _s2('V1', 257, 3, V=1),
       _s2('l2', 257, 3, l2=1)]
    # count (the inputs of these are those of 'all-terms')
    + [_s2('count-dev', 257, 3, count='dev'), _s2('count-dev2', 257, 3, count='dev2'), _s2('count-dev0', 257, 3, count='dev0'),
       _s2('empty-mask-host', 257, 3, masks='a_false'), _s2('empty-mask-dev0', 257, 3, masks='a_false', count='dev0')]
    # masks ('half' everywhere else, one all-false just above)
    + [_s2('masks-all-true', 257, 3, masks='all')]
    + [_s2('poisoned', 257, 17, poison=True)])
_S2_IN, _S2_REF = {}, {}


def s2_present(case):
    return [k for k in ('rgb', 'alb', 'wgt', 'vis', 'nrm', 'nrm_j') if k not in case['absent'] and not (k == 'nrm_j' and 'nrm' in case['absent'])]


def s2_inputs(case):
    """{name: float32 / bool CPU tensor, or None for an absent term} + 'mask' (mask_a & mask_b), 'ties' {leaf: bool mask}.  Seeded by
    the shapes alone.  Edges: ties in every L1 pair, one all-zero nrm_gt row and one scaled by 1e3 (the F.normalize floor)."""
    key = (case['N'], case['L'], case['nb'], case['V'], case['masks'], case['poison'], tuple(case['absent']))
    if key in _S2_IN:
        return _S2_IN[key]
    N, L, nb, V = case['N'], case['L'], case['nb'], case['V']
    g = torch.Generator().manual_seed(20000 + N + 7 * L + 131 * nb + 17 * V)
    t = {}
    t['rgb'], t['rgb_gt'] = _apart(g, (L, N, 3))
    t['alb'], t['alb_j'] = _apart(g, (N, 3))
    t['wgt'], t['wgt_j'] = _apart(g, (N, nb), 0.0, 3.0)
    vis = torch.rand(V, N, 3, generator=g)
    vis0, t['vis_gt'] = _apart(g, (V, N))
    unit = F.normalize(torch.randn(N, 3, generator=g), dim=-1)
    t['nrm'] = unit + 0.05 * torch.randn(N, 3, generator=g)
    t['nrm_j'] = t['nrm'] + _delta(g, (N, 3))
    t['nrm_gt'] = torch.randn(N, 3, generator=g) * (0.5 + torch.rand(N, 1, generator=g))
    if N >= 3:
        t['nrm_gt'][N // 3] = 0.0
        t['nrm_gt'][N // 2] *= 1e3
    ties = {'rgb': _tie(t['rgb'], t['rgb_gt']), 'alb': _tie(t['alb'], t['alb_j']), 'wgt': _tie(t['wgt'], t['wgt_j']),
            'vis': _tie(vis0, t['vis_gt']), 'nrm': _tie(t['nrm'], t['nrm_j'])}
    vis[..., 0] = vis0
    t['vis'] = vis
    ma, mb = torch.rand(N, generator=g) < 0.7, torch.rand(N, generator=g) < 0.7
    if N == 1 or case['masks'] == 'all':
        ma, mb = torch.ones(N, dtype=torch.bool), torch.ones(N, dtype=torch.bool)
    if case['masks'] == 'a_false':
        ma = torch.zeros(N, dtype=torch.bool)
    m = ma & mb
    if case['poison']:
        for k in S2_FLOATS:
            if k in ('rgb', 'rgb_gt', 'vis', 'vis_gt'):   # a leading light dimension
                t[k][:, ~m] = float('nan')
            else:
                t[k][~m] = float('nan')
    present = s2_present(case)
    for k in ('rgb', 'alb', 'wgt', 'vis', 'nrm'):
        if k not in present:
            for name in S2_FLOATS:
                if name == k or name.startswith(k + '_'):
                    t[name] = None
    if 'nrm_j' not in present:
        t['nrm_j'] = None
    t.update(mask_a=ma, mask_b=mb, mask=m, ties=ties)
    _S2_IN[key] = t
    return t


def s2_scales(case):
    """(inv_denom [6], weight [6], count_dev or None) as psnerf_amd.stage2.loss.fused_losses hands them to the kernels."""
    count = int(s2_inputs(case)['mask'].sum())
    L, nb, V = case['L'], case['nb'], case['V']
    count_dev = {'host': None, 'dev': float(count), 'dev2': 2.0 * count, 'dev0': 0.0}[case['count']]
    c = 1.0 if count_dev is not None else float(max(count, 1))
    inv = [1.0 / (c * L * 3), 1.0 / (c * 3), 1.0 / (c * nb), 1.0 / (c * V), 1.0 / (c * 3), 1.0 / (c * 3)]
    if count_dev is None and count == 0:
        inv = [0.0] * 6   # the reference returns 0 for every term of an empty mask
    return inv, list(S2_WEIGHT), count_dev


def s2_args(t, conv=lambda k, v: v):
    return [None if t[k] is None else conv(k, t[k]) for k in S2_FLOATS]


def s2_reference(case, dtype):
    """-> float64 ndarrays: 'terms' [6], 'total' and d_<leaf> of G_UP * total for every present leaf, evaluated in ``dtype``."""
    key = (case['id'], dtype)
    if key not in _S2_REF:
        t = s2_inputs(case)
        inv, w, count_dev = s2_scales(case)
        lv = {k: _leaf(t[k], dtype) for k in S2_LEAVES}
        args = s2_args(t, lambda k, v: lv[k] if k in lv else v.to(dtype))
        terms, total = stage2_loss(*args, t['mask_a'], t['mask_b'], case['l2'], inv, w, count_dev)
        (total * G_UP).backward()
        res = {'terms': _f64(terms), 'total': _f64(total)}
        res.update({'d_' + k: _grad(v) for k, v in lv.items() if v is not None})
        _S2_REF[key] = res
    return _S2_REF[key]


def s2_kinks(case):
    """(elements at a kink, elements) over the present leaves: the ties, and the three elements of the all-zero nrm_gt row."""
    t = s2_inputs(case)
    n = sum(t[k].numel() for k in S2_LEAVES if t[k] is not None)
    kinks = sum(int(t['ties'][k].sum()) for k in ('rgb', 'alb', 'wgt', 'vis', 'nrm') if t[k] is not None and not (k == 'nrm' and t['nrm_j'] is None))
    return kinks + (3 if t['nrm'] is not None and case['N'] >= 3 else 0), n


# --------------------------------------------------------------------------- stage-1 losses
def stage1_loss(rgb, rgb_gt, diff, hit, normal, normal_gt, norm_mask, acc, mask_gt, mask_valid, n_rays, weights, counts=None):
    """oracle.stage1.Loss with the argument list of hip.stage1_loss_fwd: colour L1 over n_rays, smoothness = mean of diff over the hit
    rays, normal L1 per selected row, BCE(acc.clamp(0, 1), mask_gt) over mask_valid (ATen's: log terms clamped at -100, backward
    (p - t) / max((1 - p) p, 1e-12); the clamp passes a gradient only for acc inside [0, 1]).  A masked term is divided by max(count,
    1); ``counts`` (hit, norm_mask, mask_valid) replaces the local counts (data parallelism).  -> terms [5], the last the total."""
    w_full, w_grad, w_norm, w_mask = weights
    z = rgb.new_zeros(())
    cnt = lambda i, m: max(float(m.sum()) if counts is None else float(counts[i]), 1.0)
    l_rgb = (rgb - rgb_gt).abs().sum() / float(n_rays) if w_full != 0.0 else z
    l_grad = diff[hit].sum() / cnt(0, hit) if (diff is not None and w_grad != 0.0) else z
    loss = w_full * l_rgb + w_grad * l_grad
    l_n = l_m = z
    if normal is not None:
        l_n = (normal[norm_mask] - normal_gt[norm_mask]).abs().sum() / cnt(1, norm_mask)
        loss = loss + w_norm * l_n
    if acc is not None:
        l_m = F.binary_cross_entropy(acc[mask_valid].clamp(0, 1), mask_gt[mask_valid], reduction='sum') / cnt(2, mask_valid)
        loss = loss + w_mask * l_m
    return torch.stack([l_rgb, l_grad, l_n, l_m, loss])


S1_WEIGHTS = (0.9, 0.5, 0.25, 2.0)
S1_COUNT_SCALE = (2.0, 3.0, 4.0)   # the 'terms' route: what the all-reduce stands in for, a different factor per count
S1_LEAVES = ('rgb', 'diff', 'normal', 'acc')


def _s1(id, N, **kw):
    """absent: 'diff' / 'normal' / 'acc' handed in as None; masks: 'mixed' or 'empty' (all three); route: 'finish' (one call) or
    'terms' (finish=False, sums[4:7] scaled by S1_COUNT_SCALE, stage1_loss_terms); acc: 'inside' or 'edges'."""
    d = dict(id=id, N=N, n_rays=N, absent=(), weights=S1_WEIGHTS, masks='mixed', route='finish', acc='inside')
    d.update(kw)
    return d


# forward: min(ceil(N / 256), 64) blocks
S1_CASES = (
    # one thread | a partial block | two blocks | the training size | exactly the 64 blocks of the cap | the grid-stride loop | five passes
    [_s1('N%d' % N, N) for N in (1, 255, 257, 4096, 16384, 16684, 70001)]
    + [_s1('N4096-rays2N', 4096, n_rays=8192)]
    + [_s1('no-' + k, 257, absent=(k,)) for k in ('diff', 'normal', 'acc')]
    + [_s1('w_full0', 257, weights=(0.0,) + S1_WEIGHTS[1:]), _s1('w_grad0', 257, weights=(0.9, 0.0, 0.25, 2.0))]
    + [_s1('empty-masks', 257, masks='empty')]
    + [_s1('terms-route-N257', 257, route='terms'), _s1('terms-route-N16684', 16684, route='terms')]
    # the clamp edges: gradients of order 1e12, which under the max-normalised bound hide every other element of the case
    + [_s1('acc-edges', 64, acc='edges')])
S1_ACC_EDGES = (0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -20, -0.1, 1.1)
S1_GT_EDGES = (0.0, 0.3, 1.0)
_S1_IN, _S1_REF = {}, {}


def s1_inputs(case):
    """{name: CPU tensor or None} + 'ties'.  acc is drawn from [0.02, 0.98], one value in ten from 0.01 .. 0.1 outside [0, 1]."""
    key = (case['N'], case['masks'], case['acc'], tuple(case['absent']))
    if key in _S1_IN:
        return _S1_IN[key]
    N = case['N']
    g = torch.Generator().manual_seed(30000 + N)
    r = lambda *s: torch.rand(*s, generator=g)
    t = {}
    t['rgb'], t['rgb_gt'] = _apart(g, (N, 3))
    t['diff'] = r(N) * 0.5
    t['normal'], t['normal_gt'] = _apart(g, (N, 3), -1.0, 1.0)
    ties = {'rgb': _tie(t['rgb'], t['rgb_gt']), 'normal': _tie(t['normal'], t['normal_gt'])}
    acc = 0.02 + 0.96 * r(N)
    out, side, far = r(N) < 0.1, r(N) < 0.5, 0.01 + 0.09 * r(N)
    t['acc'] = torch.where(out, torch.where(side, -far, 1.0 + far), acc)
    t['mask_gt'] = (r(N) > 0.5).float()
    t['hit'], t['norm_mask'], t['mask_valid'] = r(N) > 0.3, r(N) > 0.5, r(N) > 0.2
    if N == 1:
        t['hit'], t['norm_mask'], t['mask_valid'] = (torch.ones(1, dtype=torch.bool) for _ in range(3))
    if case['acc'] == 'edges':
        pairs = [(a, b) for a in S1_ACC_EDGES for b in S1_GT_EDGES]
        t['acc'][:len(pairs)] = torch.tensor([a for a, _ in pairs], dtype=torch.float64).float()
        t['mask_gt'][:len(pairs)] = torch.tensor([b for _, b in pairs])
        t['mask_valid'][:len(pairs)] = True
    if case['masks'] == 'empty':
        t['hit'], t['norm_mask'], t['mask_valid'] = (torch.zeros(N, dtype=torch.bool) for _ in range(3))
    if 'diff' in case['absent']:
        t['diff'] = None
    if 'normal' in case['absent']:
        t['normal'] = t['normal_gt'] = t['norm_mask'] = None
    if 'acc' in case['absent']:
        t['acc'] = t['mask_gt'] = t['mask_valid'] = None
    t['ties'] = ties
    _S1_IN[key] = t
    return t


S1_ARGS = ('rgb', 'rgb_gt', 'diff', 'hit', 'normal', 'normal_gt', 'norm_mask', 'acc', 'mask_gt', 'mask_valid')


def s1_counts(case):
    """The (hit, norm_mask, mask_valid) counts the terms and the backward divide by: None = the local ones."""
    if case['route'] != 'terms':
        return None
    t = s1_inputs(case)
    return [s * (0.0 if t[k] is None else float(t[k].sum())) for s, k in zip(S1_COUNT_SCALE, ('hit', 'norm_mask', 'mask_valid'))]


def s1_need(case):
    """The gradients ops.Stage1Losses.backward asks the kernel for."""
    t, w = s1_inputs(case), case['weights']
    return {k for k, on in (('rgb', w[0] != 0.0), ('diff', t['diff'] is not None and w[1] != 0.0), ('normal', t['normal'] is not None and w[2] != 0.0),
                            ('acc', t['acc'] is not None and w[3] != 0.0)) if on}


def s1_reference(case, dtype):
    """-> float64 ndarrays: 'terms' [5] and d_<leaf> of G_UP * total for the present leaves."""
    key = (case['id'], dtype)
    if key not in _S1_REF:
        t = s1_inputs(case)
        lv = {k: _leaf(t[k], dtype) for k in S1_LEAVES}
        args = [lv[k] if k in lv else (t[k] if t[k] is None or t[k].dtype == torch.bool else t[k].to(dtype)) for k in S1_ARGS]
        terms = stage1_loss(*args, case['n_rays'], case['weights'], s1_counts(case))
        (terms[4] * G_UP).backward()
        res = {'terms': _f64(terms)}
        res.update({'d_' + k: _grad(v) for k, v in lv.items() if v is not None})
        _S1_REF[key] = res
    return _S1_REF[key]


def s1_kinks(case):
    t = s1_inputs(case)
    n = sum(t[k].numel() for k in S1_LEAVES if t[k] is not None)
    kinks = int(t['ties']['rgb'].sum()) + (0 if t['normal'] is None else int(t['ties']['normal'].sum()))
    return kinks + (0 if t['acc'] is None else int(((t['acc'] == 0) | (t['acc'] == 1)).sum())), n


# --------------------------------------------------------------------------- surface normals
def surface_normals(g, hit, eps=1e-5):
    """oracle.stage1.Renderer: n = g / (|g| + eps) for the 2 N rows of g (surface points, then their neighbours); normal_pred = n
    where the ray hit, else 0; diff_norm = |n - n_neighbour|.  -> (normal_pred [N,3], diff_norm [N])."""
    N = hit.shape[0]
    n = g / (g.norm(2, dim=1).unsqueeze(-1) + eps)
    return torch.where(hit.unsqueeze(-1), n[:N], torch.zeros_like(n[:N])), torch.norm(n[:N] - n[N:], dim=-1)


# (N, hit: 'mixed' / 'all' / 'none', upstream: 'both' / 'norm_pred' / 'diff', edges: 'pair' = one pair with identical g (N >= 255) /
# 'zero' = also a row with |g| = 0 in either half).  At a zero row dg = dn / eps is of order 1e5: under the max-normalised bound it
# would hide every other element of its case (as the clamp edges of acc do), so the zero rows have cases of their own.
SN_CASES = ([(N, 'mixed', 'both', 'pair') for N in (1, 255, 257, 5000)]
            + [(257, 'all', 'both', 'pair'), (257, 'none', 'both', 'pair'), (257, 'mixed', 'norm_pred', 'pair'), (257, 'mixed', 'diff', 'pair')]
            + [(257, 'mixed', 'both', 'zero'), (257, 'mixed', 'diff', 'zero')])
SN_MIN_G, SN_MIN_DIFF = 0.05, 1e-2
_SN_IN, _SN_REF = {}, {}


def sn_id(spec):
    return 'N%d-hit_%s-d_%s-%s' % spec


def sn_inputs(spec):
    """g [2N,3] with |g| in [0.05, 2.05], the neighbours by rejection until |n - n_neighbour| >= 1e-2 in float64, and the edges of
    the case.  + hit, the upstream gradients, 'zero' (bool over the rows of g) and 'same' (bool over the pairs)."""
    N, hit_kind, _, edges = spec
    key = (N, hit_kind, edges)
    if key in _SN_IN:
        return _SN_IN[key]
    g = torch.Generator().manual_seed(40000 + N)
    a = F.normalize(torch.randn(N, 3, generator=g), dim=-1) * (SN_MIN_G + 2.0 * torch.rand(N, 1, generator=g))
    b = a.clone()
    todo = torch.ones(N, dtype=torch.bool)
    for _ in range(50):
        k = int(todo.sum())
        if k == 0:
            break
        step = F.normalize(torch.randn(k, 3, generator=g), dim=-1) * a[todo].norm(dim=-1, keepdim=True) * (0.05 + 0.3 * torch.rand(k, 1, generator=g))
        b[todo] = a[todo] + step
        with torch.no_grad():
            d = surface_normals(torch.cat([a, b]).double(), torch.ones(N, dtype=torch.bool))[1]
        todo = (d < 2 * SN_MIN_DIFF) | (b.norm(dim=-1) < SN_MIN_G)
    assert not todo.any()
    gf = torch.cat([a, b])
    zero, same = torch.zeros(2 * N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    if N >= 255:
        if edges == 'zero':
            zero[3] = zero[N + 11] = True
            gf[zero] = 0.0
        same[5] = True
        gf[N + 5] = gf[5]
    hit = {'mixed': torch.rand(N, generator=g) > 0.3, 'all': torch.ones(N, dtype=torch.bool), 'none': torch.zeros(N, dtype=torch.bool)}[hit_kind]
    if N == 1:
        hit = torch.ones(1, dtype=torch.bool)
    _SN_IN[key] = dict(g=gf, hit=hit, d_norm_pred=torch.randn(N, 3, generator=g), d_diff=torch.randn(N, generator=g), zero=zero, same=same)
    return _SN_IN[key]


def sn_reference(spec, dtype):
    """-> float64 ndarrays: normal_pred, diff_norm, dg of (normal_pred * d_norm_pred).sum() + (diff_norm * d_diff).sum() restricted
    to the upstream gradients of the case."""
    key = (spec, dtype)
    if key not in _SN_REF:
        t = sn_inputs(spec)
        gf = _leaf(t['g'], dtype)
        pred, diff = surface_normals(gf, t['hit'])
        obj = gf.new_zeros(())
        if spec[2] in ('both', 'norm_pred'):
            obj = obj + (pred * t['d_norm_pred'].to(dtype)).sum()
        if spec[2] in ('both', 'diff'):
            obj = obj + (diff * t['d_diff'].to(dtype)).sum()
        obj.backward()
        _SN_REF[key] = {'normal_pred': _f64(pred), 'diff_norm': _f64(diff), 'dg': _grad(gf)}
    return _SN_REF[key]


# --------------------------------------------------------------------------- Adam over flat buffers
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def adam_scalars(lr, step, beta1=BETA1, beta2=BETA2):
    """(neg_step_size, bias_correction2_sqrt) of torch.optim.Adam at its ``step``-th step (1-based), in float64."""
    return -lr / (1.0 - beta1 ** step), float(np.sqrt(1.0 - beta2 ** step))


def adam_update(p, g, m, v, beta1, beta2, eps, neg_step, bc2_sqrt):
    """The comment above adam_flat_kernel = torch/optim/adam.py::_multi_tensor_adam (no amsgrad, no weight decay).  -> (p, m, v)."""
    m = m + (1.0 - beta1) * (g - m)
    v = v * beta2 + (1.0 - beta2) * g * g
    den = v.sqrt() / bc2_sqrt + eps
    return p + neg_step * (m / den), m, v


ADAM_LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025)          # tails of 1 - 3 elements, one block of 256 x 4, one element more or less
ADAM_ALIGN = ((0, 0), (0, 1), (1, 1), (2, 0))          # (offset % 4, grad_offset % 4): only the first takes the float4 path
ADAM_BIG = 4096 * 1024 + 1029                          # more than the 4096 blocks of the cap cover in one pass, and a tail of one
# name -> [(length, alignment)]: 7 and 4 are coprime, so 28 segments hold every combination once and 17 every length and alignment
ADAM_CASES = {
    'seg17-2launches': [(ADAM_LENGTHS[i % 7], ADAM_ALIGN[i % 4]) for i in range(17)],
    'seg33-3launches': [(ADAM_LENGTHS[i % 7], ADAM_ALIGN[i % 4]) for i in range(33)],
    'grid-stride': [(ADAM_BIG, (0, 0)), (1025, (1, 1))],
}
ADAM_STEPS = 3
_ADAM = {}


def adam_case(name):
    """Flat buffers with gaps between the segments, the layout, and per step the gradients and per-segment scalars:
    dict(p, m, v [total]; segs [(offset, grad_offset, n)]; grads [steps][g_total]; scalars [steps][(neg_step, bc2_sqrt) per segment];
    inside (bool [total]); still (bool [total]: g = m = v = 0 throughout -- the parameter must not move)).  Segment i has its own
    learning rate and starts at its own step count; the magnitudes of g run from 1e-8 to 1e3, m and v to match."""
    if name in _ADAM:
        return _ADAM[name]
    g = torch.Generator().manual_seed(50000 + len(ADAM_CASES[name]))
    segs, cur, gcur = [], 0, 0
    for n, (a, ga) in ADAM_CASES[name]:
        off, goff = cur + 1, gcur + 2                     # at least one element between two segments, in either buffer
        off += (a - off) % 4
        goff += (ga - goff) % 4
        assert off % 4 == a and goff % 4 == ga
        segs.append((off, goff, n))
        cur, gcur = off + n, goff + n
    total, gtotal = cur + 3, gcur + 5
    scale = 10.0 ** (torch.rand(total, generator=g) * 11.0 - 8.0)
    p = torch.randn(total, generator=g)
    m = scale * torch.randn(total, generator=g) * 0.3
    v = scale * scale * torch.rand(total, generator=g) * 0.5
    inside, still = torch.zeros(total, dtype=torch.bool), torch.zeros(total, dtype=torch.bool)
    for off, _, n in segs:
        inside[off:off + n] = True
        still[off:off + n:7] = True
    m[still], v[still] = 0.0, 0.0
    grads, scalars = [], []
    for k in range(ADAM_STEPS):
        gr = torch.randn(gtotal, generator=g)
        for off, goff, n in segs:
            gr[goff:goff + n] *= scale[off:off + n]
            gr[goff:goff + n][still[off:off + n]] = 0.0
        grads.append(gr)
        scalars.append([adam_scalars(1e-3 * (1 + i % 3), (i % 4) + k + 1) for i in range(len(segs))])
    _ADAM[name] = dict(p=p, m=m, v=v, segs=segs, grads=grads, scalars=scalars, inside=inside, still=still, refs={})
    return _ADAM[name]


def adam_reference(name, dtype):
    """-> float64 ndarrays p, m, v [total] after ADAM_STEPS steps of adam_update on the segments, evaluated in ``dtype``."""
    case = adam_case(name)
    if dtype not in case['refs']:
        p, m, v = (case[k].to(dtype).clone() for k in ('p', 'm', 'v'))
        for gr, sc in zip(case['grads'], case['scalars']):
            gr = gr.to(dtype)
            for (off, goff, n), (ns, bc) in zip(case['segs'], sc):
                s = slice(off, off + n)
                p[s], m[s], v[s] = adam_update(p[s], gr[goff:goff + n], m[s], v[s], BETA1, BETA2, ADAM_EPS, ns, bc)
        case['refs'][dtype] = {'p': _f64(p), 'm': _f64(m), 'v': _f64(v)}
    return case['refs'][dtype]


# --------------------------------------------------------------------------- SparseAdam on table rows
def row_adam_step_size(lr, step, beta1=BETA1, beta2=BETA2):
    """torch.optim.SparseAdam: lr sqrt(1 - beta2^step) / (1 - beta1^step), in float64."""
    return lr * float(np.sqrt(1.0 - beta2 ** step)) / (1.0 - beta1 ** step)


def row_adam_update(p, g, m, v, idx, beta1, beta2, eps, step_size):
    """The comment above row_adam_kernel = torch's sparse_adam on the rows named in idx (once each, however often named); every other
    row of p, m and v stays as it is.  g: the dense gradient [rows, cols].  -> (p, m, v)."""
    rows = torch.unique(idx)
    rows = rows[rows < p.shape[0]]
    p, m, v = p.clone(), m.clone(), v.clone()
    gr = g[rows]
    m[rows] = m[rows] + (gr - m[rows]) * (1.0 - beta1)
    v[rows] = v[rows] + (gr * gr - v[rows]) * (1.0 - beta2)
    p[rows] = p[rows] + (m[rows] / (v[rows].sqrt() + eps)) * (-step_size)
    return p, m, v


# name -> ([(rows, cols)] tables of one launch, n_idx, index range).  256 rows = one block, 257 = two; 256 indices = one pass through
# LDS, 257 and 600 = the chunked pass; four tables = PSN_ROW_ADAM_MAX, the grid sized by the largest
ROW_ADAM_CASES = {
    'rows1-idx1': ([(1, 3), (1, 1)], 1, 1), 'rows1-idx9': ([(1, 3)], 9, 1), 'rows50-idx9': ([(50, 3), (50, 1)], 9, 50),
    'rows256-idx256': ([(256, 3), (256, 1)], 256, 256), 'rows257-idx257': ([(257, 3), (257, 1)], 257, 257),
    'rows1000-idx600': ([(1000, 3), (1000, 1)], 600, 1000), 'rows1000-idx0': ([(1000, 3), (1000, 1)], 0, 1000),
    'four-tables': ([(1000, 3), (257, 1), (1000, 2), (257, 5)], 257, 257),
}
ROW_ADAM_STEPS = 3
_ROW = {}


def row_adam_case(name):
    """dict(tables [(p, m, v)], steps [(idx int64 [n_idx] drawn with replacement and with one row named twice, [dense gradient per table], [step size per
    table])]).  Table i has its own learning rate; the moments start away from zero."""
    if name in _ROW:
        return _ROW[name]
    shapes, n_idx, hi = ROW_ADAM_CASES[name]
    g = torch.Generator().manual_seed(60000 + 7 * n_idx + hi + len(shapes))
    tables = [(torch.randn(r, c, generator=g), torch.randn(r, c, generator=g) * 0.1, torch.rand(r, c, generator=g) * 0.01) for r, c in shapes]
    steps = []
    for k in range(ROW_ADAM_STEPS):
        idx = torch.randint(0, hi, (n_idx,), generator=g)
        if n_idx >= 2:
            idx[-1] = idx[0]   # at least one row named twice
        steps.append((idx, [torch.randn(r, c, generator=g) for r, c in shapes],
                      [row_adam_step_size(5e-3 * (i + 1), k + 1) for i in range(len(shapes))]))
    _ROW[name] = dict(tables=tables, steps=steps, refs={})
    return _ROW[name]


def row_adam_reference(name, dtype):
    """-> [(p, m, v) float64 ndarrays per table] after ROW_ADAM_STEPS steps, and the bool [rows] of the rows ever touched."""
    case = row_adam_case(name)
    if dtype not in case['refs']:
        tabs = [tuple(t.to(dtype) for t in tab) for tab in case['tables']]
        touched = [torch.zeros(tab[0].shape[0], dtype=torch.bool) for tab in tabs]
        for idx, grads, sizes in case['steps']:
            tabs = [row_adam_update(p, gr.to(dtype), m, v, idx, BETA1, BETA2, ADAM_EPS, ss) for (p, m, v), gr, ss in zip(tabs, grads, sizes)]
            for tch in touched:
                tch[idx[idx < tch.shape[0]]] = True
        case['refs'][dtype] = ([tuple(_f64(t) for t in tab) for tab in tabs], touched)
    return case['refs'][dtype]


# --------------------------------------------------------------------------- the bound, on the CPU
def ratio(x, truth):
    """max over the elements of |x - truth| / (RTOL |truth| + RTOL max|truth|); 0 for an all-zero truth that is matched exactly."""
    x, truth = np.asarray(x, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    if truth.size == 0:
        return 0.0
    d, bound = np.abs(x - truth), RTOL * np.abs(truth) + RTOL * float(np.abs(truth).max())
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where((d == 0) & (bound == 0), 0.0, d / bound)
    return float(np.where(np.isnan(r), np.inf, r).max())
