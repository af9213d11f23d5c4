"""The cases and references of tests/ray_cases.py, checked without a GPU: the composite cases cover every row of the
dispatcher's table (recomputed from a pure-Python copy of its conditions) and straddle every kernel's grid cap; the float32
reference arithmetic stays inside the cap that keeps the GPU test's allowance from hiding a failure (measured ratios printed);
deliberately wrong formulations are rejected by the GPU test's own bound; the constructed crossing profiles give what their
construction says; and the forced sample depths do reach the sort.  The per-ray kernels' float32 definitions (secant step,
stage-1 rays) stay within half the float64 bound, their edge inputs give what the construction says (f_mid == 0 moves the high end,
under == 0 is a miss, x = w is the last pixel, exact ties round half to even, a coordinate of +-box is inside), and the wrong forms
-- the y axis over fy, the strict box test, floor(x + 0.5) for rint -- are rejected.  78 tests, 40 s (the composite references)."""
import numpy as np
import pytest
import torch

from tests import ray_cases as rc
from tests.helpers import assert_vs_truth, truth_ratios

MAX_SHARE, MAX_WORST = 0.02, 4.0   # the fp32 reference: share of its elements beyond half the bound, worst element / bound


def test_dispatch_table_is_covered():
    """Every row of the table: (mode, kernel, E, vector) -> the n_samples that must reach it, aligned unless said otherwise."""
    have = {}
    for c in rc.ALL_FWD + rc.ALL_BWD:
        have.setdefault((c['mode'],) + rc.case_path(c), set()).add((c['S'], c['mis']))
    need = {
        # blocked, weights
        ('w', 'blocked', 1, False): [1, 7, 63], ('w', 'blocked', 2, False): [65, 127], ('w', 'blocked', 2, True): [128],
        ('w', 'blocked', 4, False): [129, 130], ('w', 'blocked', 4, True): [132], ('w', 'blocked', 8, False): [300],
        ('w', 'blocked', 8, True): [512], ('w', 'blocked', 16, False): [1000], ('w', 'blocked', 16, True): [1024],
        ('w', 'multi16', 4, True): [4, 60, 64], ('w', 'multi32', 4, True): [68, 96, 124],
        ('nw', 'flat', 2, False): [65, 96, 127, 128],
        ('nw', 'blocked', 1, False): [64], ('nw', 'blocked', 4, False): [129], ('nw', 'blocked', 4, True): [256],
        ('op', 'acc4', 4, True): [64], ('op', 'acc4', 8, True): [128],
        ('op', 'blocked', 1, False): [16, 48, 63], ('op', 'blocked', 2, True): [96], ('op', 'blocked', 4, True): [256],
        ('bwd', 'bwd', 1, False): [1, 7, 64], ('bwd', 'bwd', 2, False): [65, 96, 128], ('bwd', 'bwd', 4, False): [130],
        ('bwd', 'bwd', 8, False): [300], ('bwd', 'bwd', 16, False): [1024],
    }
    for row, sizes in need.items():
        for S in sizes:
            assert (S, None) in have.get(row, ()), 'no aligned case reaches %s at S = %d' % (row, S)
    # the fall-backs that only an offset view reaches: non-vector although S % E == 0; acc4 -> blocked; multi-ray -> blocked
    offset = {('w', 'blocked', 2, False): [128, 96], ('w', 'blocked', 4, False): [132], ('w', 'blocked', 8, False): [512],
              ('w', 'blocked', 16, False): [1024], ('w', 'blocked', 1, False): [64, 7], ('nw', 'blocked', 4, False): [256],
              ('nw', 'flat', 2, False): [96], ('op', 'blocked', 1, False): [64], ('op', 'blocked', 2, False): [128, 96],
              ('op', 'blocked', 4, False): [256], ('bwd', 'bwd', 2, False): [96], ('bwd', 'bwd', 4, False): [130]}
    for row, sizes in offset.items():
        for S in sizes:
            for mis in (('alpha',) if row[0] == 'op' else ('alpha', 'rgb')):
                assert (S, mis) in have.get(row, ()), 'no case with an offset %s reaches %s at S = %d' % (mis, row, S)
    # every small case at every small N, every backward case in the four forms (tensors() lists them)
    for mode, sizes in rc.FWD_S.items():
        for S in sizes:
            assert {c['N'] for c in rc.FWD_CASES if (c['mode'], c['S']) == (mode, S)} == set(rc.SMALL_N)
    c = rc.BWD_CASES[0]
    assert {n.split()[1] for n, _, _, _ in rc.tensors(c, rc.reference(c))} == set(rc.BWD_FORMS)
    print('\n%d dispatcher rows, %d forward + %d backward cases' % (len(have), len(rc.ALL_FWD), len(rc.ALL_BWD)))


def test_grid_caps_are_straddled():
    """Per kernel: C + 1, C + 5 and 2 C + 3 rays -- a second pass that only some waves run, a last pass in either register set
    (2 and 3 passes), a ray count that is no multiple of the rays per wave, and for the four-rays-per-wave kernels a last wave
    whose first ray alone is live (C + 5: rays C + 4 .. C + 7 belong to one wave, only C + 4 exists)."""
    for mode, S, kernel in rc.CAP_FWD + [('bwd', rc.CAP_BWD_S, 'bwd')]:
        C, rpw = rc.CAP[kernel], rc.RAYS_PER_WAVE[kernel]
        cases = [c for c in rc.FWD_CAP_CASES + rc.BWD_CAP_CASES if (c['mode'], c['S']) == (mode, S)]
        assert sorted(c['N'] for c in cases) == [C + 1, C + 5, 2 * C + 3]
        for c in cases:
            assert rc.case_path(c)[0] == kernel
            assert c['N'] % rpw != 0 or rpw == 1
        assert sorted(-(-c['N'] // C) for c in cases) == [2, 2, 3]   # passes of the busiest wave: last in r1, r1, r0
        if rpw == 4:
            assert (C + 5) - (C + 4) == 1   # the wave at base C + 4 has rq = 0 live and rq = 1..3 not
    # nothing else is large
    big = [c for c in rc.ALL_FWD + rc.ALL_BWD if c['N'] > 4000]
    assert len(big) == 3 * (len(rc.CAP_FWD) + 1) and all(c in rc.FWD_CAP_CASES + rc.BWD_CAP_CASES for c in big)


def _cap_figures(c, scale):
    """[(tensor, share beyond half the bound, worst / bound, finite)] of the fp32 reference of a case at a given scale."""
    out = []
    for name, t, r, atol in rc.tensors(c, rc.reference(c)):
        _, r_ref, _, n_half, _ = truth_ratios(r, r, t, rc.RTOL * scale, atol if isinstance(atol, str) else atol * scale)
        out.append((name, n_half / r_ref.size, float(r_ref.max()), bool(np.isfinite(r).all() and np.isfinite(t).all())))
    return out


def test_reference_arithmetic_within_cap():
    """The allowance of assert_vs_truth is what the fp32 reference shows against float64, so the reference must be good: per case
    and tensor finite, at most 2 % of its elements beyond half the bound, worst element at most 4 x the bound.  Prints the
    worst figures per n_samples and tensor."""
    worst = {}
    for c in rc.FWD_CASES + rc.BWD_CASES + rc.FWD_CAP_CASES + rc.BWD_CAP_CASES:
        for name, share, w, finite in _cap_figures(c, rc.scale_of(c['S'])):
            assert finite, (rc.case_id(c), name)
            assert share <= MAX_SHARE and w <= MAX_WORST, '%s %s: %.2f %% beyond half the bound, worst x%.2f' % (
                rc.case_id(c), name, 100 * share, w)
            k = (c['S'], name.split()[0])
            worst[k] = (max(worst.get(k, (0, 0))[0], share), max(worst.get(k, (0, 0))[1], w))
    print('\nfloat32 reference vs float64: S, scale, tensor, worst share beyond half the bound, worst |error| / bound')
    for (S, name), (share, w) in sorted(worst.items()):
        print('  S %4d  x%d  %-10s %5.2f %%  %5.2f' % (S, rc.scale_of(S), name, 100 * share, w))


def test_scale_is_the_smallest_power_of_two():
    """The long-ray sizes carry a recorded scale, a power of two; one above 1 must miss the cap at half its value on some case (so
    it is not generous).  That no smaller S needs one is the test above."""
    assert set(rc.SCALE) == {512, 1000, 1024} and all(S in rc.FWD_S['w'] for S in rc.SCALE)
    for S, scale in sorted(rc.SCALE.items()):
        assert scale >= 1 and scale & (scale - 1) == 0
        if scale > 1:
            figs = [f for c in rc.FWD_CASES + rc.BWD_CASES if c['S'] == S for f in _cap_figures(c, scale // 2)]
            assert [f for f in figs if f[1] > MAX_SHARE or f[2] > MAX_WORST], 'S = %d meets the cap at scale %d already' % (S, scale // 2)


def _as_kernel(c, variant):
    """{tensor name of rc.tensors: float32 values} of the explicit formulation (correct, or with one mistake) on a case with colours."""
    inp = rc.make_inputs(c)
    if c['kind'] == 'fwd':
        o = {w: rc.explicit_formulation(inp, w == 'white', variant) for w in ('black', 'white')}
        return {'w': o['black']['w'], 'acc': o['black']['acc'], 'rgb_black': o['black']['rgb'], 'rgb_white': o['white']['rgb']}
    out = {}
    for f in ('white', 'black', 'no_d_acc'):
        o = rc.explicit_formulation(inp, f != 'black', variant, d_acc=f != 'no_d_acc')
        out['d_alpha ' + f], out['d_rgb ' + f] = o['d_alpha'], o['d_rgb']
    return out


def _failures(c, variant):
    """Names of the tensors of case c on which the formulation fails the GPU test's check."""
    got, bad = _as_kernel(c, variant), []
    for name, t, r, atol in rc.tensors(c, rc.reference(c)):
        if name in got:
            try:
                assert_vs_truth(name, got[name], r, t, *rc.bound(c, atol))
            except AssertionError:
                bad.append(name)
    return bad


COLOUR_CASES = [c for c in rc.FWD_CASES + rc.BWD_CASES if c['mode'] in ('w', 'bwd')]


def test_a_correct_second_formulation_passes():
    """The composite written out by hand in float32 (cumprod / cumsum, another operation order than autograd's) passes the GPU
    test's check on every case: the bound admits an independent correct evaluation."""
    for c in COLOUR_CASES:
        assert _failures(c, None) == [], rc.case_id(c)


@pytest.mark.parametrize('variant', rc.WRONG_VARIANTS)
def test_wrong_formulation_is_rejected(variant):
    """Each mistake, evaluated in float32 in place of the kernel, fails assert_vs_truth on the tensors it touches -- the
    evidence that the GPU test would fail on a kernel that is wrong in this way."""
    touched = {'inclusive': 'w', 'no_carry': 'w', 'bg_sign': 'rgb_white', 'bg_acc': 'rgb_white', 'channels': 'd_rgb',
               'suffix_incl': 'd_alpha', 'no_eps': 'w'}[variant]
    hits = {}
    for c in COLOUR_CASES:
        bad = _failures(c, variant)
        if any(b.startswith(touched) for b in bad):
            hits.setdefault(c['S'], []).append(c['N'])
    print('\n%s: rejected on %s at S -> N: %s' % (variant, touched, sorted(hits.items())))
    assert hits
    if variant == 'no_carry':   # every S above one chunk, at every N
        for S in rc.FWD_S['w']:
            assert (sorted(hits.get(S, [])) == sorted(rc.SMALL_N)) == (S > 64), S
    if variant in ('inclusive', 'bg_sign', 'bg_acc', 'channels', 'suffix_incl'):   # (S = 1: one sample shows no ordering)
        sizes = rc.FWD_S['w'] if touched in ('w', 'rgb_white') else rc.BWD_S
        assert set(hits) >= {S for S in sizes if S > 1}
    if variant == 'no_eps':
        # zero-then-saturated rays: the weight at sample k moves by k 1e-6 against a bound of at most 1.1e-5 -> caught once a
        # ray has more than about ten (near-)zero samples in front, so at every S from 60 on (k is uniform in [0, S))
        assert set(hits) >= {S for S in rc.FWD_S['w'] if S >= 60}
        # and the gradient divides by t = 1 - a = 0 on the saturated samples: not finite, never passes
        c = [c for c in rc.BWD_CASES if (c['N'], c['S']) == (37, 96)][0]
        assert any(b.startswith('d_alpha') for b in _failures(c, variant))


# ----------------------------------------------------------------------------------------------------------- first crossing
@pytest.mark.parametrize('M', rc.FC_M)
def test_crossing_profiles_give_what_their_construction_says(M):
    """The tensor formulation on the full list of profiles of this M: the mask and the bracket of every ray are what the
    profile was built to give (so the reference that the kernel is held to is itself pinned), finite values only."""
    c = rc.crossing_case(M, max(rc.FC_N))
    occ = c['occ']
    assert torch.isfinite(occ).all() and len(set(c['names'])) == len(rc.crossing_profiles(M))
    val = occ - rc.FC_TAU
    mask, first_free, (dl, dh, fl, fh) = rc.first_crossing_reference(val, c['u'], c['omu'], rc.FC_NEAR, c['far'])
    for i, (name, m) in enumerate(zip(c['names'], c['expect'])):
        assert bool(mask[i]) == (m >= 0), name
        assert bool(first_free[i]) == bool(occ[i, 0] < rc.FC_TAU), name
        if m >= 0:
            m2 = min(m + 1, M - 1)
            assert float(fl[i]) == float(val[i, m]) < 0 < float(fh[i]) == float(val[i, m2]), name
            assert float(dl[i]) == float(rc.FC_NEAR * c['omu'][m] + c['far'][i] * c['u'][m]) <= float(dh[i]), name
    assert int(mask.sum()) >= 2 and int((~mask).sum()) >= 2
    names = ' | '.join(sorted(set(c['names'])))
    for key in ('all free', 'all occupied', 'free->occupied at 0', 'one ulp below / above tau') + (
            ('occupied->free->occupied', 'exactly tau') if M >= 3 else ()) + (('free->occupied->free->occupied',) if M >= 4 else ()) + (
            ('changes at 0 and 64', 'free->occupied at 62', 'free->occupied at 63', 'free->occupied at 64', 'free->occupied at 65')
            if M >= 128 else ()):
        assert key in names, key


def test_crossing_small_ray_counts_take_different_profiles():
    for M in rc.FC_M:
        seen = set()
        for N in rc.FC_N:
            c = rc.crossing_case(M, N)
            assert c['occ'].shape == (N, M) and 33 <= float(c['far'].min()) and float(c['far'].max()) <= 34
            seen |= set(c['names'])
        assert len(seen) == len(rc.crossing_profiles(M))


# ------------------------------------------------------------------------------------------------------------ sample points
@pytest.mark.parametrize('c0,c1,N,noise', rc.SP_CASES)
def test_sample_cases_reach_the_sort(c0, c1, N, noise):
    """Every case with an outer segment has at least 8 rays (every ray, if it has fewer than 8) whose concatenated depths are
    not non-decreasing before the sort, so the kernel's rank selection runs by construction.  (1, 1) is the exception by
    arithmetic: its sequence is [near, dnp] with dnp >= near, which no depth can put out of order.  All three forced kinds are
    present, and the sorted reference is non-decreasing."""
    case = rc.sample_case(c0, c1, N, noise)
    dist, far = case['dist'], case['far']
    n_forced = min(N, rc.SP_FORCED)
    assert int((dist - rc.SP_DELTA > far).sum()) >= min(8, N)
    if N > 8:
        assert bool((dist <= rc.SP_NEAR + rc.SP_DELTA).any()) and bool(((dist < far) & (dist + rc.SP_DELTA > far)).any())
    mixed = case['flags']['mixed']   # the forced rays are hit rays, the last ray of a case is a miss ray
    assert bool(mixed[:max(1, n_forced - 1)].all()) and (N == 1 or not bool(mixed[-1]))
    if c1:
        n = rc.non_monotone_rays(case, c0, c1)
        print('\n(%d, %d) N = %d: %d rays not non-decreasing before the sort' % (c0, c1, N, n))
        if c1 >= 2:
            assert n >= min(8, N)
        else:
            assert n == 0
        d = rc.hit_depths(dist, far, rc.SP_NEAR, rc.SP_DELTA, c1, c0, rc.lin(c1)[0], rc.lin(c0)[0])
        assert bool((d[:, 1:] >= d[:, :-1]).all())
    ref = rc.sample_reference(case, c0, c1, case['flags']['mixed'])
    assert ref.shape == (N, c0 + c1, 3) and bool(torch.isfinite(ref).all())


# ================================================================================= the per-ray kernels around the root finder
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize('n', rc.PR_N)
def test_secant_step_definition_and_its_edge_rays(n):
    """float32 against float64 on the regular rays over the initial step and three updates (d_pred and p_mid, ATOL_UNIT: within
    half the bound); f_mid == 0 moves the HIGH end; d_low == d_high stays where it is; f_low == f_high gives inf or NaN."""
    c = rc.secant_case(n, 0.5 if n % 2 else 0.3)
    reg = np.ones(n, dtype=bool)
    if n >= 8:
        reg[[3, 4]] = False
    st32 = st64 = {k: c[k] for k in ('d_low', 'd_high', 'f_low', 'f_high')}
    d32 = d64 = None
    for step in range(4):
        occ = None if step == 0 else c['occ'][step - 1]
        before = st32
        st32, d32, p32 = rc.secant_step_definition(st32, occ, c['tau'], d32, c['origin'], c['direction'])
        st64, d64, p64 = rc.secant_step_definition(st64, occ, c['tau'], d64, c['origin'], c['direction'], np.float64)
        for name, a, t in (('d_pred', d32[reg], d64[reg]), ('p_mid', p32[reg], p64[reg])):
            _, r_ref, _, _, _ = truth_ratios(a, a, t, rc.RTOL, rc.ATOL_UNIT)
            assert float(r_ref.max()) <= 0.5, (n, step, name, float(r_ref.max()))
        if n >= 8 and step > 0:
            assert st32['d_high'][2] == before_d[2] and st32['f_high'][2] == 0 and st32['d_low'][2] == before['d_low'][2]
        if n >= 8:
            assert d32[3] == c['d_low'][3] and not np.isfinite(d32[4]) and (step > 0 or np.isinf(d32[4]))
            assert d32[5] == (0.5 if step == 0 else d32[5])
        before_d = d32
    assert np.isfinite(d32[reg]).all()


@pytest.mark.parametrize('scene', rc.RAY_SCENES)
@pytest.mark.parametrize('n', rc.PR_N)
def test_stage1_rays_definition_within_half_the_bound_and_fy_rejected(n, scene):
    pix, K, W, radius = rc.rays_case(n, scene)
    c32, d32, f32, u32 = rc.stage1_rays_definition(pix, K, W, radius)
    c64, d64, f64, u64 = rc.stage1_rays_definition(pix, K, W, radius, np.float64)
    assert (np.abs(u64) >= rc.RAY_UNDER_MIN).all() and np.array_equal(u32 > 0, u64 > 0) and np.array_equal(_bits(c32), _bits(c64))
    for name, a, t, atol in (('rays', d32, d64, rc.ATOL_UNIT), ('far', f32, f64, 'max')):
        _, r_ref, _, n_allowed, _ = truth_ratios(a, a, t, rc.RTOL, atol)
        assert n_allowed == 0 and float(r_ref.max()) <= 0.5, (name, float(r_ref.max()))
    if n > 1:
        assert {'outside': 0 < (f32 == 0).sum() < n, 'inside': (f32 > 0).all(), 'behind': (f32 == 0).all() and (u32 > 0).any()}[scene]
    # both axes over fy instead of fx: rejected by the bound on the directions
    bad = rc.stage1_rays_definition(pix, K, W, radius, wrong='fy')
    with pytest.raises(AssertionError):
        assert_vs_truth('rays fy', bad[1], d32, d64, rc.RTOL, rc.ATOL_UNIT)
    # a 3 x 3 camera matrix is the same definition
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(rc.stage1_rays_definition(pix, K[:3, :3], W, radius), (c32, d32, f32, u32)))


def test_stage1_rays_explicit_sign_of_under():
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 70.0, 66.0, 31.5, 23.25
    for cam, r2, far in rc.RAY_UNDER_EXPLICIT:
        W = np.eye(4, dtype=np.float32)
        W[:3, 3] = cam
        c, d, f, under = rc.stage1_rays_definition(np.array([[31.5, 23.25]], dtype=np.float32), K, W, np.sqrt(np.float64(r2)))
        assert d.tolist() == [[0.0, 0.0, 1.0]] and under[0] == np.float32(r2) - (np.float32(np.dot(cam, cam)) - np.float32(cam[2]) ** 2)
        assert f[0] == (far if far is not None else np.sqrt(under[0])) and (far is not None or f[0] > 0)


@pytest.mark.parametrize('n', rc.PR_N)
def test_surface_points_definition_table(n):
    d_pred, flags, cam, rays = rc.surface_case(n)
    d_i, dists, obj, pts = rc.surface_points_definition(d_pred, flags, cam, rays)
    if n >= 16:
        # flags 3 (crossing, starts free): the depth; flags 2 (no crossing): inf -> dist 1, no object; bit 1 clear: 0 -> dist 0
        want = {(3, 0): (0.75, 0.75, True), (3, 1): (0.0, 0.0, False), (3, 2): (np.inf, 1.0, False), (2, 0): (np.inf, 1.0, False),
                (1, 0): (0.0, 0.0, False), (0, 3): (0.0, 0.0, False)}
        for (f, v), (di, dist, o) in want.items():
            i = 4 * f + v
            assert (d_i[i], dists[i], bool(obj[i])) == (di, dist, o), (f, v)
        assert np.isnan(d_i[15]) and dists[15] == 1.0 and not obj[15]
    assert np.array_equal(pts, cam + rays * dists[:, None]) and 0 < obj.sum() + (n > 1) <= n


@pytest.mark.parametrize('h,w', rc.TG_SIZES)
def test_targets_definition_ties_bounds_and_wrong_rounding(h, w):
    c = rc.targets_case(h, w, 257)
    iy, ix, inside, fx, fy = rc.nearest_index(c['pix'], h, w)
    pix = c['pix']
    # x = w and y = h are the last pixel (2 w / w - 1 = 1 with align_corners=True); x = -1 (from three columns on), w + 1, h + 1 and
    # (w + 5, -3) are outside: zeros.  An image of one column (row) has fx = x * 0: every x (y) is inside.
    assert inside[[0, 1, 3, 4]].all() and (iy[1], ix[1]) == (h - 1, w - 1) and ix[3] == w - 1 and iy[4] == h - 1
    rgb = rc.targets_definition(c)[0]
    assert np.array_equal(rgb[1], c['img'][:, h - 1, w - 1]) and np.array_equal(rgb[3], c['img'][:, 0, w - 1])
    out = [k for k, on in ((2, w >= 3), (5, w >= 2 or h >= 2), (12, w >= 2), (13, h >= 2)) if on]
    assert not inside[out].any() and (rgb[out] == 0).all() and ((h, w) == (1, 1) or len(out) >= 2)
    # the exact ties of even sizes: fx = (w - 1) / 2 exactly, rounded half to even
    if w % 2 == 0:
        assert fx[6] == (w - 1) / 2.0 and ix[6] == 2 * round((w - 1) / 4.0)
    if h % 2 == 0:
        assert fy[7] == (h - 1) / 2.0 and iy[7] == 2 * round((h - 1) / 4.0)
    bad = rc.targets_definition(c, wrong='floor')[0]
    if (h, w) == (6, 8):      # 2.5 -> 2 (rint) but 3 (floor(x + 0.5)): the wrong rounding reads another pixel
        assert iy[7] == 2 and not np.array_equal(bad, rgb)
    # the angle mask: n2 == cos exactly is kept, one ulp below is dropped
    full = rc.targets_definition(c, want_normal=True, use_angle=True)
    plain = rc.targets_definition(c, want_normal=True, use_angle=False)
    assert full[3][0] and plain[3][0] and plain[3][1] and (not full[3][1] or (h, w) == (1, 1))
    assert np.array_equal(full[4], plain[4]) and full[4].dtype == np.float32


@pytest.mark.parametrize('case', rc.SH_CASES, ids=lambda c: 'ns%d-nl%d-S%d-%s' % (c[0], c[1], c[2], c[5]))
def test_shadow_definition_counts_and_strict_box_rejected(case):
    ns, nl, S, lnear, box, kind = case
    surf, ldir, u, omu = rc.shadow_case(*case)
    rows, pts = rc.shadow_points_definition(surf, ldir, u, omu, lnear, rc.SH_LFAR, box)
    total = ns * nl * S
    assert total % 64 != 0 or total == 0
    assert {'random': 0 < len(rows) < total or total <= 1, 'all': len(rows) == total, 'none': len(rows) == 0,
            'edge': 0 < len(rows) < total}[kind]
    if kind == 'edge':
        # step 0 of light 0: the point is the surface point; +-box inside, one ulp beyond outside
        first = [(0 * ns + s) * S for s in range(8)]
        assert [r in rows for r in first] == [True, True, True, False, False, False, True, False]
        srows, _ = rc.shadow_points_definition(surf, ldir, u, omu, lnear, rc.SH_LFAR, box, strict=True)
        assert len(srows) < len(rows) and not any(r in srows for r in first)
