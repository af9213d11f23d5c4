"""The stage-1 ray pipeline, kernel path by kernel path: psn_composite_fwd / _bwd (csrc/composite.hip) against the oracle's
formulas in float64, psn_first_crossing and psn_sample_points / _flagged (csrc/sample.hip) bit for bit against the torch
formulations of the reference -- on the cases of tests/ray_cases.py, whose coverage tests/test_ray_cpu.py asserts without a GPU.

Composite.  Every row of the dispatcher's table (six forward kernels, vector and non-vector row access, E = 1 .. 16, backward
E = 1 .. 16) at N = 1, 5, 37, 130 rays; every forward case with a black and a white background, every backward case in four
forms (white, black, d_acc = None, rgb = None).  Per kernel three ray counts around its grid cap C (C + 1, C + 5, 2 C + 3: the
second and third pass of the double-buffered grid-stride loops, the last pass in either register set, a last wave with one live
ray): flat 16385 / 16389 / 32771 x 96, opacity-only 131073 / 131077 / 262147 x 128 and x 64, several rays per wave 32769 / 32773 /
65539 x 64 and x 96, blocked 16385 / 16389 / 32771 x 130, backward 16385 / 16389 / 32771 x 96.  Offset inputs: alpha alone and rgb
alone as contiguous views that start one float into their buffer (4 mod 16), which takes the non-vector blocked kernel in place
of the vector, the several-rays and the four-rays-per-wave ones; the weights output is allocated by hip.composite_fwd and cannot
be offset through it.

Bound: helpers.assert_vs_truth, rtol 1e-5, atol ATOL_UNIT for w / rgb / acc and 'max' for the gradients (x SCALE of ray_cases for
S >= 512, measured to be 1): the kernel may have as many elements beyond the bound as the float32 CPU reference has beyond half of
it and a worst element of max(1, 2 x the reference's worst).  test_ray_cpu.py caps that reference (finite, <= 2 % beyond half
the bound, worst <= 4 x) and shows that seven wrong formulations fail this very check.

The per-ray kernels around the root finder (last section): psn_secant_step, psn_stage1_rays, psn_surface_points, psn_stage1_targets and
psn_shadow_points bit for bit against the numpy float32 definitions of ray_cases.py at n = 1, 255, 256, 257 and n = 0, on the edge
inputs listed there; d_pred, p_mid, the ray directions and far also against float64 (rtol 1e-5; ATOL_UNIT, 'max' for far).  Measured
on an MI355X: every output equals its definition bit for bit.  With align_corners=True the pixel positions x = w and y = h are
the LAST pixel, not outside (x = w + 1 is): the tests assert what the reference's formula gives.
"""
import numpy as np
import pytest
import torch

from tests import ray_cases as rc
from tests.helpers import assert_vs_truth

pytestmark = pytest.mark.gpu
_WORST = {}   # (kernel, tensor) -> (worst r_hip, r_ref of that case, case)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _WORST:
        print('\n==== composite kernels vs float64: worst r_hip (the reference arithmetic in the same case), in units of the bound ====')
        for (kernel, name), (rh, rr, where) in sorted(_WORST.items()):
            print('%-22s %-10s r_hip %7.3f  r_ref %7.3f  (%s)' % (kernel, name, rh, rr, where))


def path_name(c):
    kernel, E, vec = rc.case_path(c)
    return '%s E=%d%s' % (kernel, E, ' vec' if vec and kernel == 'blocked' else '')


def check(c, name, got, truth, ref, atol, key=None):
    assert got.shape == truth.shape, '%s %s: shape %s vs %s' % (rc.case_id(c), name, tuple(got.shape), truth.shape)
    rtol, atol = rc.bound(c, atol)
    rh, rr = assert_vs_truth('%s %s' % (rc.case_id(c), name), got.cpu().numpy(), ref, truth, rtol, atol)
    print('%s %-16s r_hip %.3f r_ref %.3f' % (rc.case_id(c), name, rh, rr))
    k = (path_name(c), key or name)
    if rh > _WORST.get(k, (-1.0,))[0]:
        _WORST[k] = (rh, rr, rc.case_id(c))


def on_device(c, cuda):
    """The case's inputs on the device; the tensor named by c['mis'] as a view one float into its buffer."""
    inp = rc.make_inputs(c)
    d = {k: (None if v is None else v.to(cuda)) for k, v in inp.items()}
    if c['mis'] is not None:
        k = {'alpha': 'alpha', 'rgb': 'rgb'}[c['mis']]
        d[k] = rc.offset_by_one(inp[k], cuda)
        assert torch.equal(d[k].cpu(), inp[k])
    for k in ('alpha', 'rgb'):
        if d[k] is not None and c['mis'] != k:
            assert d[k].data_ptr() % 16 == 0
    return d


@pytest.mark.parametrize('c', rc.ALL_FWD, ids=rc.case_id)
def test_composite_forward_vs_float64(cuda, c):
    from psnerf_amd import hip
    d = on_device(c, cuda)
    ref = rc.reference(c)
    t, r = ref[torch.float64], ref[torch.float32]
    N, S, mode = c['N'], c['S'], c['mode']
    for white in (False, True):
        w, out, acc = hip.composite_fwd(d['alpha'], d['rgb'], white, need_weights=mode == 'w')
        bg = 'white' if white else 'black'
        if mode == 'w':
            check(c, 'w (%s)' % bg, w, t['w'], r['w'], rc.ATOL_UNIT, key='w')
        else:
            assert w is None
        check(c, 'acc (%s)' % bg, acc, t['acc'], r['acc'], rc.ATOL_UNIT, key='acc')
        if mode == 'op':
            assert out is None
        else:
            check(c, 'rgb_' + bg, out, t['rgb_' + bg], r['rgb_' + bg], rc.ATOL_UNIT)


@pytest.mark.parametrize('c', rc.ALL_BWD, ids=rc.case_id)
def test_composite_backward_vs_float64(cuda, c):
    from psnerf_amd import hip
    d = on_device(c, cuda)
    ref = rc.reference(c)
    t, r = ref[torch.float64], ref[torch.float32]
    for form in rc.BWD_FORMS:
        if form == 'no_rgb':
            da, dc = hip.composite_bwd(d['alpha'], None, None, d['c2'], True)
            assert dc is None
        else:
            da, dc = hip.composite_bwd(d['alpha'], d['rgb'], d['c1'], None if form == 'no_d_acc' else d['c2'], form != 'black')
            check(c, 'd_rgb ' + form, dc, t[form]['d_rgb'], r[form]['d_rgb'], 'max')
        check(c, 'd_alpha ' + form, da, t[form]['d_alpha'], r[form]['d_alpha'], 'max')


# one case per (mode, kernel, E, vector, offset): the N = 37 cases
KNOWN = list({(c['mode'],) + rc.case_path(c) + (c['mis'],): c for c in rc.FWD_CASES + rc.FWD_MIS_CASES if c['N'] == rc.MIS_N}.values())


@pytest.mark.parametrize('c', KNOWN, ids=rc.case_id)
def test_composite_known_answers_on_every_path(cuda, c):
    """All-zero opacities: acc == 0 and, under a white background, rgb == 1 exactly.  All-one opacities: w[:, 0] == 1 exactly and
    w[:, 1:] <= 2e-6 (w_1 = eps = 1e-6, the rest eps^2 and below); without a weights output the same statement on their sum,
    1 <= acc <= 1 + 2e-6."""
    from psnerf_amd import hip
    d = on_device(c, cuda)
    need_w = c['mode'] == 'w'
    place = (lambda x: rc.offset_by_one(x.cpu(), cuda)) if c['mis'] == 'alpha' else (lambda x: x)
    w, out, acc = hip.composite_fwd(place(torch.zeros_like(d['alpha'])), d['rgb'], True, need_weights=need_w)
    assert float(acc.abs().max()) == 0
    if need_w:
        assert float(w.abs().max()) == 0
    if d['rgb'] is not None:
        assert float((out - 1).abs().max()) == 0
    w, out, acc = hip.composite_fwd(place(torch.ones_like(d['alpha'])), d['rgb'], False, need_weights=need_w)
    if need_w:
        assert float((w[:, 0] - 1).abs().max()) == 0 and (c['S'] == 1 or float(w[:, 1:].abs().max()) < 2e-6)
    assert float(acc.min()) >= 1 and float(acc.max()) <= 1 + 2e-6
    if d['rgb'] is not None:   # the first sample's colour, and at most 2e-6 of the others
        assert float((out - d['rgb'][:, 0]).abs().max()) <= 2e-6


# ----------------------------------------------------------------------------------------------------------- first crossing
@pytest.mark.parametrize('M,N', rc.FC_CASES)
def test_first_crossing_on_constructed_profiles(cuda, M, N):
    """Bit for bit against the tensor formulation evaluated on the CPU: both flag bits on every ray, the four bracket rows where
    the mask bit is set, (0, 1, -1, 1) elsewhere."""
    from psnerf_amd import hip
    c = rc.crossing_case(M, N)
    val = c['occ'] - rc.FC_TAU
    mask, first_free, rows = rc.first_crossing_reference(val, c['u'], c['omu'], rc.FC_NEAR, c['far'])
    bracket, flags = hip.first_crossing(c['occ'].to(cuda), c['far'].to(cuda), c['u'].to(cuda), c['omu'].to(cuda), rc.FC_NEAR, rc.FC_TAU)
    bracket, flags = bracket.cpu(), flags.cpu()
    assert bracket.shape == (4, N) and flags.shape == (N,)
    bad = lambda sel: [c['names'][i] for i in sel.nonzero().reshape(-1).tolist()]
    assert torch.equal((flags & 1).bool(), mask), bad((flags & 1).bool() != mask)
    assert torch.equal((flags & 2).bool(), first_free), bad((flags & 2).bool() != first_free)
    assert not bool((flags & ~3).any())
    for row, (ref, benign) in enumerate(zip(rows, (0.0, 1.0, -1.0, 1.0))):
        want = torch.where(mask, ref, torch.full_like(ref, benign))
        assert torch.equal(bracket[row], want), 'bracket row %d: %s' % (row, bad(bracket[row] != want))


# ------------------------------------------------------------------------------------------------------------ sample points
@pytest.mark.parametrize('c0,c1,N,noise', rc.SP_CASES)
def test_sample_points_flagged_and_indexed(cuda, c0, c1, N, noise):
    """Mixed, all-hit and all-miss flags: the flagged launch == the two indexed launches == the CPU formulation, bit for bit;
    the depths of the first rays force the reference's sort to reorder (asserted on the CPU in test_ray_cpu.py)."""
    from psnerf_amd import hip
    case = rc.sample_case(c0, c1, N, noise)
    S = case['S']
    dev = {k: case[k].to(cuda) for k in ('cam', 'rays', 'far', 'dist')}
    nz = None if case['noise'] is None else case['noise'].to(cuda)
    u0, u1, um = rc.lin(c0, cuda), (rc.lin(c1, cuda) if c1 else None), rc.lin(S, cuda)
    for tag, flags in case['flags'].items():
        ref = rc.sample_reference(case, c0, c1, flags)
        fl = flags.to(cuda)
        out_f = torch.full((N, S, 3), float('nan'), device=cuda)
        hip.sample_points_flagged(dev['cam'], dev['rays'], dev['dist'], dev['far'], fl, out_f, rc.SP_NEAR, rc.SP_DELTA, u0, u1, um, noise=nz)
        out_i = torch.full((N, S, 3), float('nan'), device=cuda)
        hit_idx, miss_idx = fl.nonzero(as_tuple=True)[0], (~fl).nonzero(as_tuple=True)[0]
        if miss_idx.numel():
            hip.sample_points(dev['cam'], dev['rays'], dev['far'], out_i, False, rc.SP_NEAR, um, idx=miss_idx,
                              noise=None if nz is None else nz[miss_idx].contiguous())
        if hit_idx.numel():
            hip.sample_points(dev['cam'], dev['rays'], dev['far'], out_i, True, rc.SP_NEAR, u0, idx=hit_idx, dist=dev['dist'],
                              delta=rc.SP_DELTA, u1=u1, noise=None if nz is None else nz[hit_idx].contiguous())
        for name, out in (('flagged', out_f), ('indexed', out_i)):
            out = out.cpu()
            assert torch.equal(out, ref), '%s, %s flags: %d of %d rays differ, max |diff| = %g' % (
                name, tag, int((out != ref).any(-1).any(-1).sum()), N, float((out - ref).abs().max()))


# ================================================================================= the per-ray kernels around the root finder
# psn_secant_step, psn_stage1_rays, psn_surface_points, psn_stage1_targets, psn_shadow_points against the numpy float32 definitions
# of tests/ray_cases.py, bit for bit, at n = 1, 255, 256, 257 (one thread per ray, 256 per workgroup) and n = 0 (nothing launched);
# the real-number outputs also against float64 (helpers.assert_vs_truth, rtol 1e-5, ATOL_UNIT for unit-scale values).
PR_NAN = 0x7FC54321


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(got, want):
    """Equal int32 bits, NaN in the same places (a NaN's payload is not part of any formulation)."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want, dtype=got.dtype)
    if got.shape != want.shape:
        return False
    if got.dtype != np.float32:
        return bool(np.array_equal(got, want))
    ng, nw = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(ng, nw) and np.array_equal(got.view(np.int32)[~ng], want.view(np.int32)[~ng]))


def _nan_tensor(shape, cuda):
    return torch.full(shape, PR_NAN, dtype=torch.int32, device=cuda).view(torch.float32)


def _is_nan_fill(t):
    return bool((t.view(torch.int32) == PR_NAN).all())


@pytest.mark.parametrize('n', rc.PR_N)
def test_secant_step_equals_definition(cuda, n):
    """The initial step (occ = NULL) and three updates, the last one without a query point (p_mid = NULL): d_pred, the four bracket
    rows and p_mid bit for bit; f_mid == 0 exactly moves the high end, d_low == d_high and f_low == f_high as the definition has
    them; d_pred and p_mid of the regular rays against float64."""
    from psnerf_amd import hip
    c = rc.secant_case(n, 0.5 if n % 2 else 0.3)
    keys = ('d_low', 'd_high', 'f_low', 'f_high')
    st_dev = {k: _dev(c[k], cuda) for k in keys}
    origin, direction = _dev(c['origin'], cuda), _dev(c['direction'], cuda)
    d_pred, p_mid = _nan_tensor((n,), cuda), _nan_tensor((n, 3), cuda)
    st32 = st64 = {k: c[k] for k in keys}
    d32 = d64 = p32 = None
    reg = np.ones(n, dtype=bool)
    if n >= 8:
        reg[[3, 4]] = False
    for step in range(4):
        occ = None if step == 0 else c['occ'][step - 1]
        last = step == 3
        hip.secant_step(None if occ is None else _dev(occ, cuda), c['tau'], d_pred, st_dev['d_low'], st_dev['d_high'], st_dev['f_low'],
                        st_dev['f_high'], origin, direction, None if last else p_mid)
        p_before = p32
        st32, d32, p32 = rc.secant_step_definition(st32, occ, c['tau'], d32, c['origin'], c['direction'])
        st64, d64, p64 = rc.secant_step_definition(st64, occ, c['tau'], d64, c['origin'], c['direction'], np.float64)
        what = 'n=%d step %d' % (n, step)
        assert _same(d_pred, d32), what + ': d_pred'
        for k in keys:
            assert _same(st_dev[k], st32[k]), '%s: %s' % (what, k)
        assert _same(p_mid, p_before if last else p32), what + ': p_mid'
        assert_vs_truth(what + ' d_pred', d_pred.cpu().numpy()[reg], d32[reg], d64[reg], rc.RTOL, rc.ATOL_UNIT)
        if not last:
            assert_vs_truth(what + ' p_mid', p_mid.cpu().numpy()[reg], p32[reg], p64[reg], rc.RTOL, rc.ATOL_UNIT)
    if n >= 8:
        assert float(st_dev['f_high'][2]) == 0.0      # occ == tau: f_mid = 0 went to the HIGH end
    # n = 0: PSN_OK, nothing written
    keep = d_pred.clone()
    rc_ = hip._lib.psn_secant_step(None, 0.5, d_pred.data_ptr(), *[st_dev[k].data_ptr() for k in keys], origin.data_ptr(),
                                   direction.data_ptr(), p_mid.data_ptr(), 0, hip._stream())
    torch.cuda.synchronize()
    assert rc_ == 0 and _same(d_pred, keep.cpu().numpy())


@pytest.mark.parametrize('scene', rc.RAY_SCENES)
@pytest.mark.parametrize('n', rc.PR_N)
def test_stage1_rays_equal_definition_and_float64(cuda, n, scene):
    """cam, rays and far bit for bit with a 4 x 4 and a 3 x 3 camera matrix; rays (unit vectors) and far against float64.  The scenes:
    rays that miss the sphere (under <= 0: far = 0), an origin inside it, a sphere behind the camera (far clamped to 0)."""
    from psnerf_amd import hip
    pix, K, W, radius = rc.rays_case(n, scene)
    c32, d32, f32, _ = rc.stage1_rays_definition(pix, K, W, radius)
    _, d64, f64, _ = rc.stage1_rays_definition(pix, K, W, radius, np.float64)
    for Km in (K, K[:3, :3]):
        cam, rays, far = hip.stage1_rays(_dev(pix, cuda), _dev(Km, cuda), _dev(W, cuda), radius)
        what = '%s n=%d k_ld=%d' % (scene, n, Km.shape[0])
        assert _same(cam, c32) and _same(rays, d32), what
        assert _same(far, f32), '%s: far differs on %d rays' % (what, int((far.cpu().numpy() != f32).sum()))
        assert_vs_truth(what + ' rays', rays.cpu().numpy(), d32, d64, rc.RTOL, rc.ATOL_UNIT)
        assert_vs_truth(what + ' far', far.cpu().numpy(), f32, f64, rc.RTOL, 'max')


def test_stage1_rays_sign_of_under_and_no_rays(cuda):
    """The explicit inputs of ray_cases.RAY_UNDER_EXPLICIT: under == 0 is a miss, one ulp above it a hit with far = its root; n = 0."""
    from psnerf_amd import hip
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 70.0, 66.0, 31.5, 23.25
    pix = _dev(np.array([[31.5, 23.25]], dtype=np.float32), cuda)
    for camv, r2, far_want in rc.RAY_UNDER_EXPLICIT:
        W = np.eye(4, dtype=np.float32)
        W[:3, 3] = camv
        radius = float(np.sqrt(np.float64(r2)))
        assert float(np.float32(radius ** 2)) == r2
        want = rc.stage1_rays_definition(pix.cpu().numpy(), K, W, radius)
        cam, rays, far = hip.stage1_rays(pix, _dev(K, cuda), _dev(W, cuda), radius)
        assert _same(cam, want[0]) and _same(rays, want[1]) and _same(far, want[2]), (camv, r2)
        assert far_want is None or float(far) == far_want
    cam, rays, far = (_nan_tensor(s, cuda) for s in ((1, 3), (1, 3), (1,)))
    Kd, Wd = _dev(K, cuda), _dev(np.eye(4, dtype=np.float32), cuda)
    rc_ = hip._lib.psn_stage1_rays(pix.data_ptr(), Kd.data_ptr(), 4, Wd.data_ptr(), 1.0, 0, cam.data_ptr(), rays.data_ptr(), far.data_ptr(),
                                   hip._stream())
    torch.cuda.synchronize()
    assert rc_ == 0 and _is_nan_fill(cam) and _is_nan_fill(rays) and _is_nan_fill(far)


@pytest.mark.parametrize('n', rc.PR_N)
def test_surface_points_equal_definition(cuda, n):
    """flags {0, 1, 2, 3} x d_pred {finite, 0, +inf, NaN}: d_i, dists, obj_mask and points exactly, with and without the d_i output."""
    from psnerf_amd import hip
    d_pred, flags, cam, rays = rc.surface_case(n)
    d_i, dists, obj, pts = rc.surface_points_definition(d_pred, flags, cam, rays)
    args = [_dev(a, cuda) for a in (d_pred, flags, cam, rays)]
    got = hip.surface_points(*args, want_d=True)
    assert _same(got[0], dists) and got[1].dtype == torch.bool and _same(got[1], obj) and _same(got[2], pts) and _same(got[3], d_i)
    got = hip.surface_points(*args)
    assert len(got) == 3 and _same(got[0], dists) and _same(got[1], obj) and _same(got[2], pts)
    out = [_nan_tensor(s, cuda) for s in ((1,), (1,), (1, 3))]
    mask = torch.full((4,), 7, dtype=torch.uint8, device=cuda)
    rc_ = hip._lib.psn_surface_points(args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(), 0, out[0].data_ptr(),
                                      out[1].data_ptr(), mask.data_ptr(), out[2].data_ptr(), hip._stream())
    torch.cuda.synchronize()
    assert rc_ == 0 and all(_is_nan_fill(t) for t in out) and bool((mask == 7).all())


@pytest.mark.parametrize('n', rc.PR_N)
@pytest.mark.parametrize('h,w', rc.TG_SIZES)
def test_stage1_targets_equal_definition(cuda, h, w, n):
    """Every combination of the optional images (mask, mask_valid, norm_mask) x (no normal, normal, normal with the angle mask), at
    257 pixel positions (one combination at the other counts): integer pixels, positions outside, fractional ones, exact ties
    (half to even) and a normal whose n2 equals the threshold (kept) or lies one ulp below it (dropped)."""
    from psnerf_amd import hip
    c = rc.targets_case(h, w, n)
    d = {k: _dev(c[k], cuda) for k in ('img', 'mask', 'valid', 'nmask', 'normal', 'world', 'pix')}
    combos = [(m, v, nm, nor) for m in (True, False) for v in (True, False) for nm in (True, False) for nor in ('none', 'plain', 'angle')]
    for m, v, nm, nor in (combos if n == 257 else combos[2:3]):
        want = rc.targets_definition(c, mask=m, valid=v, nmask=nm, want_normal=nor != 'none', use_angle=nor == 'angle')
        got = hip.stage1_targets(d['pix'], d['img'], d['mask'] if m else None, d['valid'] if v else None,
                                 d['normal'] if nor != 'none' else None, d['nmask'] if nm else None,
                                 d['world'] if nor != 'none' else None, c['cos_t'] if nor == 'angle' else None, nor != 'none')
        what = '%dx%d n=%d mask=%s valid=%s norm_mask=%s normal=%s' % (h, w, n, m, v, nm, nor)
        assert got[0].shape == (n, 3) and got[2].dtype == torch.bool
        for name, g, r in zip(('rgb', 'mask_gt', 'mask_valid', 'norm_mask', 'normal_gt'), got, want):
            assert (g is None) == (r is None), '%s: %s' % (what, name)
            assert g is None or _same(g, r), '%s: %s' % (what, name)
    if n == 257 and (h, w) != (1, 1):
        full = hip.stage1_targets(d['pix'], d['img'], None, None, d['normal'], d['nmask'], d['world'], c['cos_t'], True)
        assert bool(full[3][0]) and not bool(full[3][1])     # n2 == cos: kept; one ulp below: dropped


def test_stage1_targets_refusal_and_no_pixels(cuda):
    """normal_gt without the normal image or without world_mat: PSN_E_ARG, nothing written; n = 0: PSN_OK, nothing written."""
    from psnerf_amd import hip
    c = rc.targets_case(6, 8, 257)
    d = {k: _dev(c[k], cuda) for k in ('img', 'normal', 'world', 'pix')}
    with pytest.raises(RuntimeError, match='needs the normal image and world_mat'):
        hip.stage1_targets(d['pix'], d['img'], normal=None, world_mat=d['world'], want_normal=True)
    with pytest.raises(RuntimeError, match='needs the normal image and world_mat'):
        hip.stage1_targets(d['pix'], d['img'], normal=d['normal'], world_mat=None, want_normal=True)
    # the optional OUTPUTS of the ABI (the wrapper always asks for mask_gt and mask_valid): none of them, and each alone beside rgb_gt
    full = {k: _dev(c[k], cuda) for k in ('mask', 'valid', 'nmask')}
    want = rc.targets_definition(c, want_normal=True, use_angle=True)
    lib, ptr = hip._lib, lambda t: None if t is None else t.data_ptr()
    for pick in (None, 'mask_gt', 'mask_valid', 'normal_gt', 'norm_mask'):
        outs = dict(mask_gt=_nan_tensor((257,), cuda), mask_valid=torch.full((257,), 7, dtype=torch.uint8, device=cuda),
                    normal_gt=_nan_tensor((257, 3), cuda), norm_mask=torch.full((257,), 7, dtype=torch.uint8, device=cuda))
        rgb = _nan_tensor((257, 3), cuda)
        use = {k: (v if k == pick else None) for k, v in outs.items()}
        rc_ = lib.psn_stage1_targets(d['pix'].data_ptr(), 257, 6, 8, d['img'].data_ptr(), full['mask'].data_ptr(), full['valid'].data_ptr(),
                                     d['normal'].data_ptr(), full['nmask'].data_ptr(), d['world'].data_ptr(), 1, c['cos_t'], rgb.data_ptr(),
                                     ptr(use['mask_gt']), ptr(use['mask_valid']), ptr(use['normal_gt']), ptr(use['norm_mask']), hip._stream())
        torch.cuda.synchronize()
        assert rc_ == 0 and _same(rgb, want[0]), pick
        for k, ref in zip(('mask_gt', 'mask_valid', 'norm_mask', 'normal_gt'), want[1:]):
            if k == pick and k == 'norm_mask':
                # without the normal_gt output the angle mask is not applied (it belongs to the branch that reads the normal)
                ref = rc.targets_definition(c, want_normal=False)[3]
            got = outs[k]
            if k == pick:
                assert _same(got.bool() if got.dtype == torch.uint8 else got, ref), (pick, k)
            else:
                assert _is_nan_fill(got) if got.dtype == torch.float32 else bool((got == 7).all()), (pick, k)
    rgb, ngt = _nan_tensor((257, 3), cuda), _nan_tensor((257, 3), cuda)
    rc_ = lib.psn_stage1_targets(d['pix'].data_ptr(), 257, 6, 8, d['img'].data_ptr(), None, None, None, None, d['world'].data_ptr(), 0, 0.0,
                                 rgb.data_ptr(), None, None, ngt.data_ptr(), None, hip._stream())
    torch.cuda.synchronize()
    assert rc_ != 0 and _is_nan_fill(rgb) and _is_nan_fill(ngt)
    rc_ = lib.psn_stage1_targets(d['pix'].data_ptr(), 0, 6, 8, d['img'].data_ptr(), None, None, d['normal'].data_ptr(), None,
                                 d['world'].data_ptr(), 0, 0.0, rgb.data_ptr(), None, None, ngt.data_ptr(), None, hip._stream())
    torch.cuda.synchronize()
    assert rc_ == 0 and _is_nan_fill(rgb) and _is_nan_fill(ngt)


@pytest.mark.parametrize('case', rc.SH_CASES, ids=lambda c: 'ns%d-nl%d-S%d-%s' % (c[0], c[1], c[2], c[5]))
def test_shadow_points_equal_definition(cuda, case):
    """counter == the definition's count, the sorted rows == its set, pts[k] == its point of rows[k] bit for bit (the order of the
    compacted rows is free), nothing written behind the counter: totals that are no multiple of 64 or 256, no lights, no surface
    points, coordinates exactly +-box (inside) and one ulp beyond (outside), all inside, none inside."""
    from psnerf_amd import hip
    ns, nl, S, lnear, box, kind = case
    surf, ldir, u, omu = rc.shadow_case(*case)
    rows_ref, pts_ref = rc.shadow_points_definition(surf, ldir, u, omu, lnear, rc.SH_LFAR, box)
    total = ns * nl * S
    cap = total + 5
    pts = _nan_tensor((cap, 3), cuda)
    rows = torch.full((cap,), -1, dtype=torch.int64, device=cuda)
    counter = torch.zeros(3, dtype=torch.int64, device=cuda)
    counter[0], counter[2] = -5, -7          # guards around the counter
    one = torch.zeros(3, device=cuda)        # (an empty tensor has no device pointer: a stand-in that is never read)
    sd, ld = (_dev(surf, cuda) if ns else one), (_dev(ldir, cuda) if nl else one)
    ud, od = _dev(u, cuda), _dev(omu, cuda)      # (held: a temporary's memory is handed to the next allocation)
    rc_ = hip._lib.psn_shadow_points(sd.data_ptr(), ld.data_ptr(), ns, nl, S, float(lnear), float(rc.SH_LFAR), ud.data_ptr(),
                                     od.data_ptr(), float(box), pts.data_ptr(), rows.data_ptr(), counter[1:].data_ptr(), hip._stream())
    torch.cuda.synchronize()
    k = len(rows_ref)
    assert rc_ == 0 and counter.tolist() == [-5, k, -7]
    assert _is_nan_fill(pts[k:]) and bool((rows[k:] == -1).all()), 'written behind the counter'
    got_rows = rows[:k].cpu().numpy()
    order = np.argsort(got_rows, kind='stable')
    assert np.array_equal(got_rows[order], rows_ref)
    assert _same(pts[:k].cpu().numpy()[order], pts_ref)
    if ns and nl:      # the wrapper: the same set
        p2, r2, c2 = hip.shadow_points(sd, ld, S, lnear, rc.SH_LFAR, ud, od, box)
        o2 = np.argsort(r2[:k].cpu().numpy(), kind='stable')
        assert int(c2) == k and np.array_equal(r2[:k].cpu().numpy()[o2], rows_ref) and _same(p2[:k].cpu().numpy()[o2], pts_ref)
