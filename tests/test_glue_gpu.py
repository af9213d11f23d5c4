"""The kernels that run around the fused engines, launch path by launch path, on the cases of tests/glue_cases.py (whose coverage,
restatements and comparators tests/test_glue_cpu.py checks without a GPU): csrc/pe.hip (psn_pe_encode / _jvp / _bwd, psn_app_input),
csrc/weight_norm.hip, the row, index and copy kernels of csrc/small.hip, and csrc/views.hip through hip.view_batch.

Rounded results: glue_cases.check = helpers.assert_vs_truth against the float64 truth with the fp32 restatement's measured allowance
(bounds in glue_cases' docstring).  Copies, gathers, index kernels, view_batch and the exact weight-norm cases: bit for bit.
Every output that a wrapper lets the caller pass is a view into a NaN-filled (integers: sentinel-filled) buffer whose margins are
checked after the launch, and every input a view that starts one element into its buffer, except where a path needs alignment
(the 64-column encode and the mask counter's word path, which have cases of either alignment).

Grid caps: a cap case tiles a 1024-row base; its first 1024 rows go through the bound, and the rows of EVERY pass of the capped
grid-stride loop are compared bit for bit with the base rows they repeat, one named check per pass."""
import ctypes

import numpy as np
import pytest
import torch

from tests import glue_cases as gc

pytestmark = pytest.mark.gpu
F32, F64 = gc.F32, gc.F64
SENTINEL = {torch.float32: float('nan'), torch.uint8: 0x5a, torch.int64: -0x5a5a5a5a5a5a5a5a, torch.int32: -0x5a5a5a5a}


@pytest.fixture(scope='module', autouse=True)
def _report():
    gc._WORST.clear()
    yield
    if gc._WORST:
        print('\n==== glue kernels vs float64: worst r_hip (worst r_ref of the restatement), in units of the bound ====')
        for k, (rh, rr) in sorted(gc._WORST.items()):
            print('%-18s r_hip %7.3f  r_ref %7.3f' % (k, rh, rr))


class Guard(object):
    """Outputs as views into filled buffers: alloc() hands out the view, check() asserts that nothing outside the views moved."""

    def __init__(self, device):
        self.device, self.bufs = device, []

    def alloc(self, shape, dtype=torch.float32, lead=64, as_bool=False):
        n = int(np.prod(shape))
        buf = torch.full((lead + n + 64,), SENTINEL[dtype], dtype=dtype, device=self.device)
        self.bufs.append((buf, lead, n))
        view = buf[lead:lead + n].view(*shape)
        return view.view(torch.bool) if as_bool else view

    def check(self):
        for buf, lead, n in self.bufs:
            for m in (buf[:lead], buf[lead + n:]):
                ok = torch.isnan(m).all() if buf.dtype == torch.float32 else (m == SENTINEL[buf.dtype]).all()
                assert bool(ok), 'a kernel wrote outside its output (%d elements at offset %d)' % (n, lead)

    def untouched(self, view):
        """Whether a float output still holds nothing but its fill."""
        return bool(torch.isnan(view).all())


def dev(a, device, off=1):
    """A numpy array on the device as a contiguous view that starts ``off`` elements into its buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if off == 0:
        return t.to(device)
    buf = torch.empty(t.numel() + off + 3, dtype=t.dtype, device=device)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def bits_equal(a, b):
    """Bit for bit; a NaN matches a NaN of any payload (sincosf and sinf need not agree on it)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


# ================================================================================================================= pe.hip
def _encode(hip, c, inp, cuda, mis, rows=None):
    g = Guard(cuda)
    x = dev(inp['x'], cuda)
    t = dev(inp['t'], cuda) if c['kind'] == 'jvp' else None
    if rows is not None:
        x, t = x[rows].contiguous(), (None if t is None else t[rows].contiguous())
    out = g.alloc((x.shape[0], c['stride']), lead=65 if mis else 64)
    assert (out.data_ptr() % 16 == 0) == (not mis)
    if c['kind'] == 'jvp':
        hip.pe_encode_jvp(x, t, c['nf'], c['stride'], c['scale'], out=out)
    else:
        hip.pe_encode(x, c['nf'], c['stride'], c['scale'], out=out)
    torch.cuda.synchronize()
    g.check()
    return out


def _check_passes(c, out, base):
    """Every pass of the capped grid: its rows bit-equal to the base rows they repeat."""
    rows = torch.arange(c['n'], device=out.device) % gc.BASE_ROWS
    passes = gc.pe_pass_rows(c)
    assert len(passes) >= 2
    for p, a, b in passes:
        assert bits_equal(out[a:b], base[rows[a:b]]), '%s: pass %d (rows %d .. %d) differs from the rows it repeats' % (c['id'], p + 1, a, b)


@pytest.mark.parametrize('c', gc.PE_ENC_CASES + gc.PE_JVP_CASES, ids=lambda c: c['id'])
def test_pe_encode_and_jvp(cuda, c):
    from psnerf_amd import hip
    inp = gc.pe_inputs(c)
    out = _encode(hip, c, inp, cuda, c['mis'])
    gc.check_pe(c, inp, out.cpu().numpy())
    if c['stride'] == 64:   # the 64-column kernel (sincosf) and the generic one (sinf / cosf) give the same bits
        other = _encode(hip, c, inp, cuda, not c['mis'])
        assert bits_equal(out, other), c['id'] + ': the aligned and the offset 64-column output differ'


@pytest.mark.parametrize('c', gc.PE_ENC_CAP_CASES + gc.PE_JVP_CAP_CASES, ids=lambda c: c['id'])
def test_pe_encode_and_jvp_grid_cap(cuda, c):
    from psnerf_amd import hip
    inp = gc.pe_inputs(c)
    rows = torch.from_numpy(inp['rows']).to(cuda)
    out = _encode(hip, c, inp, cuda, c['mis'], rows)
    gc.check_pe(c, inp, out[:gc.BASE_ROWS].cpu().numpy())
    _check_passes(c, out, out[:gc.BASE_ROWS])


def _bwd(hip, c, inp, cuda, rows=None):
    g = Guard(cuda)
    x, g1 = dev(inp['x'], cuda), dev(inp['g1'], cuda)
    g2 = None if inp['g2'] is None else dev(inp['g2'], cuda)
    if rows is not None:
        x, g1 = x[rows].contiguous(), g1[rows].contiguous()
    w = gc.pe_width(c['nf'])
    d_out = g1[:, 2:2 + c['stride']]                      # a column range of a wider tensor: row stride = stride + 5
    add = None if g2 is None else g2[:, 4:4 + w]          # ... and another one of another width
    assert d_out.stride(0) == c['stride'] + 5 and (add is None or add.stride(0) == w + 9)
    d_x = g.alloc((x.shape[0], 3), lead=65)
    hip.pe_encode_bwd(x, d_out, c['nf'], c['scale'], add=add, out=d_x)
    torch.cuda.synchronize()
    g.check()
    return d_x


@pytest.mark.parametrize('c', gc.PE_BWD_CASES, ids=lambda c: c['id'])
def test_pe_encode_bwd(cuda, c):
    from psnerf_amd import hip
    inp = gc.pe_inputs(c)
    gc.check_pe(c, inp, _bwd(hip, c, inp, cuda).cpu().numpy())


@pytest.mark.parametrize('c', gc.PE_BWD_CAP_CASES, ids=lambda c: c['id'])
def test_pe_encode_bwd_grid_cap(cuda, c):
    from psnerf_amd import hip
    inp = gc.pe_inputs(c)
    d_x = _bwd(hip, c, inp, cuda, torch.from_numpy(inp['rows']).to(cuda))
    gc.check_pe(c, inp, d_x[:gc.BASE_ROWS].cpu().numpy())
    _check_passes(c, d_x, d_x[:gc.BASE_ROWS])


@pytest.mark.parametrize('c', gc.APP_CASES + gc.APP_CAP_CASES, ids=lambda c: c['id'])
def test_app_input(cuda, c):
    from psnerf_amd import hip
    inp = gc.pe_inputs(c)
    g = Guard(cuda)
    p, v, nrm = (dev(inp[k], cuda) for k in ('p', 'v', 'nrm'))
    if c['n'] > gc.BASE_ROWS:
        rows = torch.from_numpy(inp['rows']).to(cuda)
        p, v, nrm = p[rows].contiguous(), v[rows].contiguous(), nrm[rows].contiguous()
    out = g.alloc((c['n'], 64))
    hip.app_input(p, v, nrm, c['nf'], out=out)
    torch.cuda.synchronize()
    g.check()
    got = out[:gc.BASE_ROWS].cpu().numpy()
    gc.check_app(c, inp, got)
    lay = gc.app_layout(c['nf'])
    bad = np.flatnonzero(~np.isfinite(got).all(1)).tolist()
    assert bad == inp['special'] and np.isfinite(got[:, :3]).all() and np.isfinite(got[:, lay['nrm'][0]:]).all()   # |v| = 0: its view columns only
    if c['nf']:   # the bands are those of psn_pe_encode on the same v^, bit for bit
        pe = hip.pe_encode(out[:gc.BASE_ROWS, 3:6].contiguous(), c['nf'], 3 + 6 * c['nf'], 1.0)
        assert bits_equal(out[:gc.BASE_ROWS, 3:lay['bands'][1]], pe)
    if c['n'] > gc.BASE_ROWS:
        _check_passes(c, out, out[:gc.BASE_ROWS])


# ======================================================================================================== weight_norm.hip
@pytest.mark.parametrize('case', gc.WN_CASES, ids=lambda c: c['id'])
def test_weight_norm(cuda, case):
    from psnerf_amd import hip
    inputs = gc.wn_inputs(case)
    g = Guard(cuda)
    vs, gs, dws = ([dev(x[k], cuda) for x in inputs] for k in range(3))
    scales = [it['scale'] for it in case['items']]
    ws = [g.alloc(v.shape, lead=65) for v in vs]
    dvs, dgs = [g.alloc(v.shape, lead=65) for v in vs], [g.alloc(a.shape, lead=65) for a in gs]
    hip.weight_norm_fwd(vs, gs, scales, out=ws)
    hip.weight_norm_bwd(vs, gs, scales, dws, out=(dvs, dgs))
    torch.cuda.synchronize()
    g.check()
    got = [dict(w=w.cpu().numpy(), dv=dv.cpu().numpy(), dg=dg.cpu().numpy()) for w, dv, dg in zip(ws, dvs, dgs)]
    gc.check_wn(case, inputs, got)
    for it, o in zip(case['items'], got):   # a zero row: NaN in that row only
        bad = {k: np.flatnonzero(~np.isfinite(o[k].reshape(it['rows'], -1)).all(1)).tolist() for k in ('w', 'dv', 'dg')}
        assert all(b == ([2] if it['kind'] == 'zero_row' else []) for b in bad.values()), bad


# ============================================================================================================== small.hip
@pytest.mark.parametrize('eps', gc.NORM_EPS)
@pytest.mark.parametrize('n', gc.NORM_N)
def test_normalize_rows(cuda, n, eps):
    from psnerf_amd import hip
    x, gr = gc.norm_inputs(n, eps)
    g = Guard(cuda)
    xd, gd = dev(x, cuda), dev(gr, cuda)
    y, dx = g.alloc((n, 3), lead=65), g.alloc((n, 3), lead=65)
    if eps == 1e-12:
        hip.normalize_rows_fwd(xd, out=y)
        hip.normalize_rows_bwd(xd, gd, out=dx)
    else:
        hip.normalize_rows_fwd(xd, eps, out=y)
        hip.normalize_rows_bwd(xd, gd, eps, out=dx)
    torch.cuda.synchronize()
    g.check()
    gc.check_norm('n%d eps%g' % (n, eps), x, gr, eps, y.cpu().numpy(), dx.cpu().numpy())


@pytest.mark.parametrize('c', gc.LR_CASES, ids=lambda c: c['id'])
def test_light_rows(cuda, c):
    from psnerf_amd import hip
    inp = gc.lr_inputs(c)
    g = Guard(cuda)
    n_idx, n_rows, mode = c['n_idx'], c['n_rows'], c['mode']
    tab, itab, idx = dev(inp['tab'], cuda), dev(inp['itab'], cuda), dev(inp['idx'], cuda)
    with_int = mode != 'dir'
    d, it = g.alloc((n_idx, 3), lead=65), (g.alloc((n_idx, 1), lead=65) if with_int else None)
    hip.light_rows_fwd(tab, itab if with_int else None, idx, out=(d, it))
    rows = inp['tab'][inp['idx']]
    gc.check('light_fwd: ' + c['id'], d.cpu().numpy(), gc.norm_fwd(rows, 1e-12, F32), gc.norm_fwd(rows, 1e-12, F64), gc.RTOL_VALUE, gc.ATOL_UNIT)
    if with_int:
        gc.check_equal(c['id'] + ': intensity rows', it.cpu(), torch.from_numpy(inp['itab'][inp['idx']]))
    g_dir = dev(inp['g_dir'], cuda) if mode != 'int' else None
    g_int = dev(inp['g_int'], cuda) if with_int else None
    dd = g.alloc((n_rows, 3), lead=65) if g_dir is not None else None
    di = g.alloc((n_rows, 1), lead=65) if g_int is not None else None
    out = hip.light_rows_bwd(tab, idx, g_dir, g_int, out=(dd, di))
    assert out[0] is dd and out[1] is di
    terms = None
    if g_dir is not None:   # the per-occurrence terms: the same device function through psn_normalize_rows_bwd, held to float64 here
        terms = hip.normalize_rows_bwd(tab[idx].contiguous(), g_dir).cpu().numpy() if n_idx else np.zeros((0, 3), F32)
        a, r, t = gc._row_scaled(terms, gc.norm_bwd(rows, inp['g_dir'], 1e-12, F32), gc.norm_bwd(rows, inp['g_dir'], 1e-12, F64))
        gc.check('light_bwd_terms: ' + c['id'], a, r, t, gc.RTOL_GRAD, gc.RTOL_GRAD)
    torch.cuda.synchronize()
    g.check()
    gc.check_lr_bwd(c, inp, terms, None if dd is None else dd.cpu().numpy(), None if di is None else di.cpu().numpy())


@pytest.mark.parametrize('c', gc.CAM_CASES, ids=lambda c: c['id'])
def test_camera_rays(cuda, c):
    from psnerf_amd import hip
    inp = gc.cam_inputs(c)
    g = Guard(cuda)
    out = g.alloc((c['n'], 3), lead=65)
    idx = None if inp['idx'] is None else dev(inp['idx'], cuda)
    hip.camera_rays(dev(inp['uv'], cuda), dev(inp['pose'], cuda), dev(inp['K'], cuda), idx, scale=c['scale'], out=out)
    torch.cuda.synchronize()
    g.check()
    gc.check('camera_rays: ' + c['id'], out.cpu().numpy(), gc.cam_values(inp, c, F32), gc.cam_values(inp, c, F64), gc.RTOL_VALUE, gc.ATOL_UNIT)


def _mask_at(a, off, cuda):
    """A byte mask as a torch.bool view ``off`` bytes behind an aligned address (any non-zero byte counts as set)."""
    buf = torch.zeros(a.size + off + 8, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(a))
    return view.view(torch.bool)


@pytest.mark.parametrize('c', gc.MC_CASES, ids=lambda c: c['id'])
def test_mask_count(cuda, c):
    from psnerf_amd import hip
    a, b = gc.mc_inputs(c)
    g = Guard(cuda)
    out = g.alloc((1,), lead=65)
    ma = _mask_at(a, c['off'][0], cuda)
    mb = None if b is None else _mask_at(b, c['off'][1], cuda)
    if c['n']:
        assert gc.mc_path(c)[0] == ('words' if (ma.data_ptr() | (0 if mb is None else mb.data_ptr())) % 8 == 0 else 'bytes')
    hip.mask_count(ma, mb, out=out)
    torch.cuda.synchronize()
    g.check()
    assert float(out) == gc.mc_truth(a, b)


@pytest.mark.parametrize('c', gc.SI_CASES, ids=lambda c: c['id'])
def test_surface_index(cuda, c):
    from psnerf_amd import hip
    byt, cap = gc.si_inputs(c)
    idx, count = hip.surface_index(_mask_at(byt, 1, cuda), cap)
    want_idx, want_count = gc.si_truth(byt, cap)
    gc.check_equal(c['id'] + ': idx', idx.cpu(), torch.from_numpy(want_idx))
    assert float(count) == want_count   # the live count, also when the list is truncated


@pytest.mark.parametrize('c', gc.II_CASES, ids=lambda c: c['id'])
def test_inverse_index(cuda, c):
    from psnerf_amd import hip
    idx, count = gc.ii_inputs(c)
    assert idx.size > 0   # (every case has a live pixel: an empty list has no device pointer to pass)
    cd = None if count is None else dev(np.array([count], F32), cuda)
    inv = hip.inverse_index(dev(idx, cuda), c['n_pix'], cd)
    gc.check_equal(c['id'], inv.cpu(), torch.from_numpy(gc.ii_truth(idx, count, c['n_pix'])))


@pytest.mark.parametrize('case', gc.C2_CASES, ids=lambda c: c['id'])
def test_copy2d_group(cuda, case):
    from psnerf_amd import hip
    g = Guard(cuda)
    pairs, want = [], []
    for i, it in enumerate(case['items']):
        rows, cols = it['rows'], it['cols']
        src_full = gc.rng(13, i, rows, cols).standard_normal((rows, it['ld_src'])).astype(F32)
        src = dev(src_full, cuda)[:, :cols]
        dst_full = g.alloc((rows, it['ld_dst']), lead=65)
        dst = dst_full[:, :cols]
        if it['one_d']:
            src, dst = src.reshape(-1), dst.reshape(-1)
            assert src.dim() == 1 and dst.data_ptr() == dst_full.data_ptr()
        exp = np.full((rows, it['ld_dst']), np.nan, F32)
        exp[:, :cols] = src_full[:, :cols]
        pairs.append((src, dst))
        want.append((dst_full, exp))
    hip.copy2d_group(pairs)
    torch.cuda.synchronize()
    g.check()
    for i, (full, exp) in enumerate(want):
        gc.check_equal('%s [%d]' % (case['id'], i), full.cpu(), torch.from_numpy(exp))   # the pad columns of dst keep their fill


# ============================================================================================================== views.hip
_TORCH_OF = {'object_mask': torch.uint8, 'surface_mask': torch.uint8, 'sampling_idx': torch.int64}


def _vb_device(c, cuda):
    t = gc.vb_tables(c['view'], c['dtype'])
    td = {k: (v if k == 'width' else dev(v, cuda, off=0 if k == 'images' else 1)) for k, v in t.items()}
    lidx, pix, pix0, vidx = gc.vb_indices(c)
    return t, td, (dev(lidx, cuda) if c['L'] else None), (None if pix is None else dev(pix, cuda)), pix0, (dev(vidx, cuda) if c['V'] else None)


@pytest.mark.parametrize('c', gc.VB_CASES, ids=lambda c: c['id'])
def test_view_batch(cuda, c):
    from psnerf_amd import hip
    t, td, lidx, pix, pix0, vidx = _vb_device(c, cuda)
    want = gc.vb_truth(c, t)
    g = Guard(cuda)
    out = {k: g.alloc(v.shape, _TORCH_OF.get(k, torch.float32), lead=65 if k not in _TORCH_OF else 64, as_bool=k.endswith('_mask')) for k, v in want.items()}
    res = hip.view_batch(td, lidx, pix, c['n'], out, pix0=pix0, vidx=vidx)
    torch.cuda.synchronize()
    g.check()
    assert res is out
    gc.check_vb(c, {k: v.cpu().numpy() for k, v in out.items()}, want)
    if 'rgb' in want:   # zero under the object mask
        off = ~want['object_mask'] if 'object_mask' in want else ~gc.vb_truth(dict(c, drop=None), t)['object_mask']
        assert not out['rgb'].cpu().numpy()[:, off].any()


def test_view_batch_without_pixels_writes_nothing(cuda):
    """The contract of include/psnerf_hip.h for n = 0: PSN_OK, no launch, NO output written -- light_direction_out included, although
    its rows do not depend on n.  (Through the C ABI: torch gives an empty rgb tensor a null pointer, which the entry point
    refuses for n_lights > 0 before it looks at n.)"""
    from psnerf_amd import hip
    c = dict(dtype='uint8', n=0, pix='range0', L=4, vis=True, V=3, view=0, drop=None)
    t, td, lidx, _, _, vidx = _vb_device(dict(c, n=1), cuda)
    g = Guard(cuda)
    outs = {k: g.alloc(s) for k, s in (('rgb', (4, 1, 3)), ('light_direction', (4, 3)), ('visibility', (4, 1)), ('vis_train_gt', (3, 1)), ('uv', (1, 2)))}
    b = hip.PsnViewBatch()
    b.images, b.image_type, b.lut, b.hw, b.width = td['images'].data_ptr(), 1, td['lut'].data_ptr(), gc.VB_HW, gc.VB_W
    b.object_mask, b.visibility, b.vis_plus, b.light_direction = (td[k].data_ptr() for k in ('object_mask', 'visibility', 'vis_plus', 'light_direction'))
    b.lidx, b.n_lights, b.vidx, b.n_vis, b.n, b.pix0 = lidx.data_ptr(), 4, vidx.data_ptr(), 3, 0, 0
    b.rgb, b.light_direction_out, b.visibility_out, b.vis_train_gt, b.uv = (outs[k].data_ptr() for k in ('rgb', 'light_direction', 'visibility', 'vis_train_gt', 'uv'))
    assert hip._lib.psn_view_batch(ctypes.addressof(b), hip._stream()) == 0
    torch.cuda.synchronize()
    g.check()
    assert all(g.untouched(v) for v in outs.values())
    b.n = 1                                   # the same descriptor with one pixel does write them
    assert hip._lib.psn_view_batch(ctypes.addressof(b), hip._stream()) == 0
    torch.cuda.synchronize()
    g.check()
    assert torch.equal(outs['light_direction'].cpu(), torch.from_numpy(t['light_direction'][gc.vb_indices(dict(c, n=1))[0]]))
    assert not any(g.untouched(v) for v in outs.values())
