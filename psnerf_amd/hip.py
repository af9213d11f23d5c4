"""ctypes binding of libpsnerf_hip.so (C ABI in include/psnerf_hip.h).

Importing this module loads the shared library and FAILS LOUDLY if it is
missing -- there is no CPU or PyTorch fallback on the product path.  The
prototypes, structs and constants are not repeated here: cabi.parse reads them
from the header at import, and a symbol the library lacks fails right there.  Wrappers
take torch tensors only as carriers of device pointers: they validate
device / dtype / contiguity, pass ``data_ptr()`` and the current HIP stream,
and raise RuntimeError with ``psn_last_error()`` on failure.
"""
import ctypes
import os

import torch

from . import cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libpsnerf_hip.so')

if not os.path.exists(LIB_PATH):
    raise ImportError(
        'psnerf_amd: %s is missing. Build it with `python -m psnerf_amd.build` (hipcc, gfx950). '
        'There is no fallback path.' % LIB_PATH)
_lib = ctypes.CDLL(LIB_PATH)

HEADER_PATH = os.path.join(_HERE, '..', 'include', 'psnerf_hip.h')
if not os.path.exists(HEADER_PATH):
    raise ImportError('psnerf_amd: %s is missing: the binding is derived from it. There is no fallback path.' % HEADER_PATH)

# The binding is DERIVED from the header (cabi.parse), nothing of it is written down here: every PSN_* #define and enumerator under its
# name without the prefix (EPI_*, ACT_*, OUT_*, W_*, IMG_*, *_MAX*, ...), every Psn* struct as a ctypes structure class and every psn_*
# prototype as SIGNATURES[name] = (restype, argtypes); pointers of every kind travel as void*.
_constants, _structs, SIGNATURES = cabi.parse(HEADER_PATH)
globals().update({_k[len('PSN_'):]: _v for _k, _v in _constants.items()})
globals().update(_structs)
MAX_LAYERS = MLP_MAX_LAYERS  # noqa: F821
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(_lib, _name)  # AttributeError here = library out of date: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


# When set to a list (bench.py), kernel wrappers that support it append
# (name, units, start_event, end_event, flops or None) recorded on the launch stream; units = rows for the MLP engines,
# algorithmic FLOPs for the grouped weight-gradient GEMM, algorithmic bytes for the composite kernels.
PROFILE_EVENTS = None


class _Prof(object):
    """``with _Prof(name, units):`` brackets one C-ABI launch with HIP events on the launch stream when PROFILE_EVENTS is
    a list (bench.py); ``units`` = rows, or algorithmic FLOPs / bytes of the launch, as the name's consumer defines."""

    def __init__(self, name, units, flops=None):
        self.name, self.units, self.flops, self.prof = name, units, flops, PROFILE_EVENTS

    def __enter__(self):
        if self.prof is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.prof is not None and exc[0] is None:
            self.e1.record()
            self.prof.append((self.name, self.units, self.e0, self.e1, self.flops))
        return False


def _check(rc, what):
    if rc != 0:
        raise RuntimeError('%s failed (%d): %s' % (what, rc, _lib.psn_last_error().decode()))


def _tptr(t, name, dtype=torch.float32, allow_none=False, contiguous=True):
    """Device pointer of a tensor, after the checks every wrapper shares: on the device, of ``dtype`` (one, or a tuple of the
    admissible ones) and contiguous.  The one validator of this module; helpers that add a shape rule call it."""
    if t is None:
        if allow_none:
            return None
        raise RuntimeError('%s: tensor required' % name)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('%s: must be a HIP device tensor (the product path has no CPU fallback)' % name)
    if t.dtype != dtype and (type(dtype) is not tuple or t.dtype not in dtype):
        want = ' or '.join(str(d)[len('torch.'):] for d in (dtype if type(dtype) is tuple else (dtype,)))
        raise RuntimeError('%s: must be %s, got %s' % (name, want, t.dtype))
    if contiguous and not t.is_contiguous():
        raise RuntimeError('%s: must be contiguous' % name)
    return t.data_ptr()


def _out(out, shape, like, name, dtype=torch.float32):
    """The output of a wrapper: a fresh tensor, or the caller's ``out`` (contiguous, of that shape and dtype, on the device of
    ``like``) -- a view into a larger buffer is fine."""
    if out is None:
        return torch.empty(shape, device=like.device, dtype=dtype)
    if not isinstance(out, torch.Tensor) or out.device != like.device or out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise RuntimeError('%s: out must be a contiguous %s device tensor of shape %s' % (name, str(dtype)[len('torch.'):], tuple(shape)))
    return out


def _eptr(t, stand_in):
    """Device pointer of a tensor that may be EMPTY: torch gives an empty tensor a null data pointer, which the entry points
    refuse before they look at the count.  An empty operand is never read, so the address of ``stand_in`` (a live tensor of
    the same call) travels in its place."""
    return t.data_ptr() if t.numel() else stand_in.data_ptr()


def _bits_ptr(t, name):
    """Device pointer of a tensor of sign-bit words ([rows, 4] int64, contiguous)."""
    if t.dim() != 2 or t.shape[1] != 4:
        raise RuntimeError('%s: sign-bit words are a contiguous int64 [rows, 4] device tensor' % name)
    return _tptr(t, name, torch.int64)


def _stream():
    # the raw handle of the current stream of the current device: torch.cuda.current_stream().cuda_stream builds a Stream object
    # through three Python layers (11 us; a step asks 30 - 65 times), the two C calls below take ~1 us
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def version():
    return _lib.psn_version()


# --------------------------------------------------------------------------- composite
def composite_fwd(alpha, rgb, white_bg, need_weights=True):
    """alpha [N,S], rgb [N,S,3] or None -> (weights [N,S] or None, rgb_out [N,3] or None, acc [N])."""
    N, S = alpha.shape
    weights = torch.empty_like(alpha) if need_weights else None
    rgb_out = torch.empty(N, 3, device=alpha.device, dtype=torch.float32) if rgb is not None else None
    acc = torch.empty(N, device=alpha.device, dtype=torch.float32)
    # algorithmic bytes: alpha 4 S (+ colour 12 S) in, weights 4 S (if kept) + rgb 12 + acc 4 out
    nbytes = N * (4 * S + (12 * S + 12 if rgb is not None else 0) + (4 * S if need_weights else 0) + 4)
    with _Prof('composite_fwd' if rgb is not None else 'composite_alpha', nbytes):
        _check(_lib.psn_composite_fwd(_tptr(alpha, 'alpha'), _tptr(rgb, 'rgb', allow_none=True), N, S, int(bool(white_bg)),
                                      _tptr(weights, 'weights', allow_none=True), _tptr(rgb_out, 'rgb_out', allow_none=True), _tptr(acc, 'acc'),
                                      _stream()), 'composite_fwd')
    return weights, rgb_out, acc


def composite_bwd(alpha, rgb, d_rgb_out, d_acc, white_bg):
    N, S = alpha.shape
    d_alpha = torch.empty_like(alpha)
    d_rgb = torch.empty_like(rgb) if rgb is not None else None
    with _Prof('composite_bwd', N * (36 * S + 16)):  # 36 S + 16 bytes per ray
        _check(_lib.psn_composite_bwd(_tptr(alpha, 'alpha'), _tptr(rgb, 'rgb', allow_none=True), _tptr(d_rgb_out, 'd_rgb_out', allow_none=True),
                                      _tptr(d_acc, 'd_acc', allow_none=True), N, S, int(bool(white_bg)), _tptr(d_alpha, 'd_alpha'),
                                      _tptr(d_rgb, 'd_rgb', allow_none=True), _stream()), 'composite_bwd')
    return d_alpha, d_rgb


# --------------------------------------------------------------------------- positional encoding
def pe_encode(x, n_freqs, out_stride=None, scale=1.0, out=None):
    """x [n,3] -> [n, out_stride] = [x, sin(2^k x), cos(2^k x)]_k, zero padded to out_stride."""
    n = x.shape[0]
    width = 3 + 6 * n_freqs
    out_stride = width if out_stride is None else out_stride
    out = _out(out, (n, out_stride), x, 'pe_encode')
    _check(_lib.psn_pe_encode(_tptr(x, 'x'), n, n_freqs, float(scale), _tptr(out, 'out'), out_stride, _stream()),
           'pe_encode')
    return out


def app_input(p, v, normal, n_freqs, out=None):
    """[Q, 64] input table of the stage-1 appearance chain: [p | gamma(v / |v|) | normal | 0] (psn_app_input)."""
    Q = p.shape[0]
    assert p.shape == v.shape == normal.shape == (Q, 3)
    out = _out(out, (Q, 64), p, 'app_input')
    if out.data_ptr() % 16:
        raise RuntimeError('app_input: out must be 16-byte aligned (the kernel stores four columns at a time)')
    p, v, normal = p.contiguous(), v.contiguous(), normal.contiguous()
    if Q:
        _check(_lib.psn_app_input(_tptr(p, 'p'), _tptr(v, 'v'), _tptr(normal, 'normal'), Q, int(n_freqs), out.data_ptr(), _stream()),
               'app_input')
    return out


def pe_encode_jvp(x, t, n_freqs, out_stride, scale=1.0, out=None):
    """J_PE(x) t: tangent t [n,3] -> [n, out_stride]."""
    n = x.shape[0]
    out = _out(out, (n, out_stride), x, 'pe_encode_jvp')
    _check(_lib.psn_pe_encode_jvp(_tptr(x, 'x'), _tptr(t, 't'), n, n_freqs, float(scale), _tptr(out, 'out'), out_stride,
                                  _stream()), 'pe_encode_jvp')
    return out


def pe_encode_bwd(x, d_out, n_freqs, scale=1.0, add=None, out=None):
    """d_out (and ``add``, a second gradient summed in first): row-major views [n, >= 3 + 6 n_freqs] -- column ranges of
    wider tensors are fine (row stride = stride(0))."""
    n = x.shape[0]
    d_x = torch.empty_like(x) if out is None else _out(out, x.shape, x, 'pe_encode_bwd')
    assert d_out.shape[1] >= 3 + 6 * n_freqs and (add is None or add.shape[1] >= 3 + 6 * n_freqs)
    _check(_lib.psn_pe_encode_bwd(_tptr(x, 'x'), _mat_ptr(d_out, 'd_out'), n, n_freqs, float(scale), _ld(d_out),
                                  None if add is None else _mat_ptr(add, 'add'), 0 if add is None else _ld(add),
                                  _tptr(d_x, 'd_x'), _stream()), 'pe_encode_bwd')
    return d_x


def geo_point_grad(p, n_freqs, scale, dz0, w0, dzs=None, ws=None, g_pe=None, g_pe2=None, d_grad=None):
    """d loss / d p [n,3] of the stage-1 geometry field (psn_geo_point_grad): J(p)^T (dz0 @ w0 + dzs @ ws) and, when g_pe and
    d_grad are given, + H(p)[g_pe + g_pe2, d_grad].  dz0 [n,h0] / dzs [n,hs]: cotangents of the pre-activations of layer 0 / of
    the skip layer; w0 [h0, >= d_pe] / ws [hs, >= d_pe]: the encoding columns of their EFFECTIVE weights; g_pe / g_pe2
    [n, >= d_pe]: d logit / d pe in one or two pieces.  Every matrix may be a column range of a wider tensor."""
    n, d_pe = p.shape[0], 3 + 6 * int(n_freqs)
    assert p.shape == (n, 3) and dz0.shape[0] == n and w0.shape[0] == dz0.shape[1] and w0.shape[1] >= d_pe
    assert (dzs is None) == (ws is None) and (g_pe is None) == (d_grad is None) and (g_pe2 is None or g_pe is not None)
    if dzs is not None:
        assert dzs.shape[0] == n and ws.shape[0] == dzs.shape[1] and ws.shape[1] >= d_pe
    for t in (g_pe, g_pe2):
        assert t is None or (t.shape[0] == n and t.shape[1] >= d_pe)
    assert d_grad is None or d_grad.shape == (n, 3)
    d_p = torch.empty(n, 3, device=p.device, dtype=torch.float32)
    if n == 0:
        return d_p
    opt = lambda t, name: (None, 0) if t is None else (_mat_ptr(t, name), _ld(t))
    (dzs_p, dzs_ld), (ws_p, ws_ld), (g_p, g_ld), (g2_p, g2_ld) = opt(dzs, 'dzs'), opt(ws, 'ws'), opt(g_pe, 'g_pe'), opt(g_pe2, 'g_pe2')
    with _Prof('geo_point_grad', n):
        _check(_lib.psn_geo_point_grad(_tptr(p, 'p'), n, int(n_freqs), float(scale), _mat_ptr(dz0, 'dz0'), _ld(dz0), dz0.shape[1],
                                       _mat_ptr(w0, 'w0'), _ld(w0), dzs_p, dzs_ld, 0 if dzs is None else dzs.shape[1], ws_p, ws_ld,
                                       g_p, g_ld, g2_p, g2_ld, _tptr(d_grad, 'd_grad', allow_none=True), _tptr(d_p, 'd_p'), _stream()),
               'geo_point_grad')
    return d_p


def sample_points(origin, direction, far, out, hit, near, u0, idx=None, dist=None, delta=0.0, u1=None, noise=None):
    """Fill rows ``idx`` (all rows if None) of out [N,S,3] with origin + direction * depth profile (psn_sample_points).
    u0 / u1: (linspace(0,1,c), 1 - linspace) pairs of device tensors."""
    n = origin.shape[0] if idx is None else idx.shape[0]
    c0 = u0[0].numel()
    c1 = 0 if u1 is None else u1[0].numel()
    assert out.shape[1] == c0 + c1 and out.is_contiguous() and (idx is None or idx.dtype == torch.int64)
    if noise is not None:
        assert noise.numel() == n * (c0 + c1)
    _check(_lib.psn_sample_points(_tptr(origin, 'origin'), _tptr(direction, 'direction'), _tptr(dist, 'dist', allow_none=True), _tptr(far, 'far'),
                                  None if idx is None else idx.data_ptr(), n, int(bool(hit)), float(near), float(delta),
                                  _tptr(u0[0], 'u0'), _tptr(u0[1], 'omu0'), c0,
                                  None if u1 is None else _tptr(u1[0], 'u1'), None if u1 is None else _tptr(u1[1], 'omu1'), c1,
                                  _tptr(noise, 'noise', allow_none=True), _tptr(out, 'out'), _stream()), 'sample_points')
    return out


def sample_points_flagged(origin, direction, dist, far, flags, out, near, delta, u0, u1, u_miss, noise=None):
    """Every ray of out [N,S,3] in one launch: hit profile where flags (bool [N]) is set, free-space profile elsewhere
    (psn_sample_points_flagged).  u0 / u1 / u_miss: (linspace, 1 - linspace) pairs; u1 may be None (S = c0)."""
    n = origin.shape[0]
    c0 = u0[0].numel()
    c1 = 0 if u1 is None else u1[0].numel()
    assert out.shape[1] == c0 + c1 == u_miss[0].numel() and out.is_contiguous()
    assert flags.dtype == torch.bool and flags.is_cuda and flags.is_contiguous() and flags.numel() == n
    if noise is not None:
        assert noise.numel() == n * (c0 + c1)
    _check(_lib.psn_sample_points_flagged(_tptr(origin, 'origin'), _tptr(direction, 'direction'), _tptr(dist, 'dist'), _tptr(far, 'far'),
                                          flags.data_ptr(), n, float(near), float(delta), _tptr(u0[0], 'u0'), _tptr(u0[1], 'omu0'), c0,
                                          None if u1 is None else _tptr(u1[0], 'u1'), None if u1 is None else _tptr(u1[1], 'omu1'), c1,
                                          _tptr(u_miss[0], 'um'), _tptr(u_miss[1], 'omum'), _tptr(noise, 'noise', allow_none=True), _tptr(out, 'out'),
                                          _stream()), 'sample_points_flagged')
    return out


# --------------------------------------------------------------------------- GEMM
_ws_cache = {}


def copy2d_group(pairs):
    """pairs: [(src, dst)] fp32 device tensors of equal shape, 1-D (contiguous) or 2-D with unit column stride (row strides
    allowed: column slices of a parameter, row blocks of a table) -> dst[...] = src[...], COPY2D_MAX pairs per launch."""
    for c0 in range(0, len(pairs), COPY2D_MAX):
        chunk = pairs[c0:c0 + COPY2D_MAX]
        arr = (PsnCopy2dItem * len(chunk))()
        for e, (src, dst) in zip(arr, chunk):
            assert src.shape == dst.shape and src.dtype == dst.dtype == torch.float32 and src.is_cuda and dst.is_cuda and src.numel() > 0
            if src.dim() == 1:
                assert src.stride(0) == 1 and dst.stride(0) == 1
                e.rows, e.cols, e.ld_src, e.ld_dst = 1, src.shape[0], src.shape[0], src.shape[0]
            else:
                assert src.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
                e.rows, e.cols, e.ld_src, e.ld_dst = src.shape[0], src.shape[1], src.stride(0), dst.stride(0)
            e.src, e.dst = src.data_ptr(), dst.data_ptr()
        _check(_lib.psn_copy2d_group(len(chunk), ctypes.addressof(arr), _stream()), 'copy2d_group')


def copy_group(pairs):
    """dst.copy_(src) for every (dst, src) pair of contiguous device tensors with equal dtype and element count, <= 24 per launch
    (psn_copy_bytes_group): the batch of a step into the input buffers of a captured HIP graph in one launch."""
    for c0 in range(0, len(pairs), COPY_BYTES_MAX):
        chunk = pairs[c0:c0 + COPY_BYTES_MAX]
        arr = (PsnCopyBytesItem * len(chunk))()
        for e, (dst, src) in zip(arr, chunk):
            assert dst.is_cuda and src.is_cuda and dst.dtype == src.dtype and dst.numel() == src.numel() and dst.is_contiguous() and src.is_contiguous()
            e.src, e.dst, e.n_bytes = src.data_ptr(), dst.data_ptr(), dst.numel() * dst.element_size()
        _check(_lib.psn_copy_bytes_group(len(chunk), ctypes.addressof(arr), _stream()), 'copy_bytes_group')


def mask_count(mask_a, mask_b=None, out=None):
    """Number of elements with mask_a & mask_b (torch.bool tensors of one size) -> float32 device tensor [1], one launch (empty
    masks included: the kernel writes the 0)."""
    assert mask_a.is_cuda and mask_a.dtype == torch.bool and mask_a.is_contiguous()
    if mask_b is not None:
        assert mask_b.is_cuda and mask_b.dtype == torch.bool and mask_b.is_contiguous() and mask_b.numel() == mask_a.numel()
    if out is None:
        out = torch.empty(1, device=mask_a.device, dtype=torch.float32)
    assert out.is_cuda and out.dtype == torch.float32 and out.numel() == 1
    _check(_lib.psn_mask_count(_eptr(mask_a, out), None if mask_b is None else _eptr(mask_b, out), mask_a.numel(), out.data_ptr(), _stream()),
           'mask_count')
    return out


def inverse_index(idx, n_pixels, count=None):
    """Pixel -> row map of an ascending index list: [n_pixels] int32, -1 where the pixel is not in idx (one launch).  count
    (float32 [1] on the device): the list is padded to a fixed length and only its first count[0] entries are real."""
    assert idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 1
    assert count is None or (count.is_cuda and count.dtype == torch.float32 and count.numel() == 1)
    inv = torch.empty(n_pixels, device=idx.device, dtype=torch.int32)
    _check(_lib.psn_inverse_index(idx.data_ptr(), idx.numel(), n_pixels, inv.data_ptr(), None if count is None else count.data_ptr(), _stream()),
           'inverse_index')
    return inv


def scatter_rows(specs, rows, inv, n_pixels, n_surf):
    """specs: [(B, C, fill)], rows: matching list of [B*Ns, C] fp32 tensors (any strides, stride-0 columns allowed) ->
    list of dense [B, N, C] tensors, one launch per 16 outputs."""
    dev = inv.device
    dense = [torch.empty(B, n_pixels, C, device=dev, dtype=torch.float32) for B, C, _ in specs]
    for c0 in range(0, len(specs), SCATTER_MAX_ITEMS):
        n = min(SCATTER_MAX_ITEMS, len(specs) - c0)
        arr = (PsnScatterItem * n)()
        for i in range(n):
            (B, C, fill), r, e = specs[c0 + i], rows[c0 + i], arr[i]
            assert r.dtype == torch.float32 and r.is_cuda and r.shape == (B * n_surf, C)
            e.rows, e.dense = r.data_ptr(), dense[c0 + i].data_ptr()
            e.row_stride, e.col_stride, e.B, e.C, e.fill = r.stride(0), r.stride(1), B, C, float(fill)
        assert inv.dtype == torch.int32 and inv.is_contiguous() and inv.numel() == n_pixels
        _check(_lib.psn_scatter_rows(n, ctypes.addressof(arr), inv.data_ptr(), n_pixels, n_surf, _stream()), 'scatter_rows')
    return dense


def surface_index(mask, capacity):
    """Ascending positions of the True elements of a 1-D bool device tensor in a FIXED-size int64 list [capacity]: entries behind
    the real ones repeat the last one (psn_surface_index; no host synchronisation).  -> (idx, count float32 [1])."""
    assert mask.is_cuda and mask.dtype == torch.bool and mask.dim() == 1 and mask.is_contiguous()
    idx = torch.empty(int(capacity), device=mask.device, dtype=torch.int64)
    count = torch.empty(1, device=mask.device, dtype=torch.float32)
    _check(_lib.psn_surface_index(_eptr(mask, idx), mask.numel(), int(capacity), idx.data_ptr(), count.data_ptr(), _stream()), 'surface_index')
    return idx, count


IMAGE_TYPES = {torch.float32: 0, torch.uint8: 1, torch.uint16: 2}


def view_batch(tables, lidx, pix, n, out, pix0=0, vidx=None):
    """One stage-2 training batch gathered from the resident tables of a view (psn_view_batch; one launch, no allocation).
    ``tables``: dict of contiguous device tensors -- 'images' [Lv, hw, 3] (float32 / uint8 / uint16), 'lut' (integer images),
    'object_mask' / 'surface_mask' [hw] bool, 'points' / 'normal' [hw, 3], optional 'visibility' [Lv, hw], 'vis_plus' [R, hw],
    'light_direction' [Lv, 3]; 'width'.  ``lidx`` [L] / ``pix`` [n] (or None: the range pix0 .. pix0 + n) / ``vidx`` [V]: device int64.
    ``out``: dict of preallocated contiguous outputs, any subset of 'rgb' [L, n, 3], 'object_mask' / 'surface_mask' [n] bool,
    'uv' [n, 2], 'points' / 'normal' [n, 3], 'visibility' [L, n], 'vis_train_gt' [V, n], 'sampling_idx' [n] int64,
    'light_direction' [L, 3]."""
    b = PsnViewBatch()
    img = tables['images']
    assert img.is_cuda and img.is_contiguous() and img.dtype in IMAGE_TYPES and img.dim() == 3 and img.shape[2] == 3
    hw = img.shape[1]
    b.images, b.image_type, b.hw, b.width = img.data_ptr(), IMAGE_TYPES[img.dtype], hw, int(tables['width'])
    if b.image_type:
        lut = tables['lut']
        assert lut.is_cuda and lut.dtype == torch.float32 and lut.is_contiguous() and lut.numel() == (256 if b.image_type == 1 else 65536)
        b.lut = lut.data_ptr()

    def table(key, shape_tail, dtype):
        t = tables.get(key)
        if t is None:
            return None
        assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape[-len(shape_tail):]) == shape_tail, key
        return t.data_ptr()
    b.object_mask, b.surface_mask = table('object_mask', (hw,), torch.bool), table('surface_mask', (hw,), torch.bool)
    b.points, b.normal = table('points', (hw, 3), torch.float32), table('normal', (hw, 3), torch.float32)
    b.visibility, b.vis_plus = table('visibility', (hw,), torch.float32), table('vis_plus', (hw,), torch.float32)
    b.light_direction = table('light_direction', (3,), torch.float32)
    L = 0 if lidx is None else int(lidx.numel())
    for t_ in (lidx, pix, vidx):
        assert t_ is None or (t_.is_cuda and t_.dtype == torch.int64 and t_.is_contiguous() and t_.dim() == 1)
    assert pix is None or pix.numel() == n
    b.lidx, b.n_lights = (None if lidx is None else lidx.data_ptr()), L
    b.pix, b.pix0, b.n = (None if pix is None else pix.data_ptr()), int(pix0), int(n)
    V = 0 if (vidx is None or 'vis_train_gt' not in out) else int(vidx.numel())
    b.vidx, b.n_vis = (vidx.data_ptr() if V else None), V
    want = {'rgb': ((L, n, 3), torch.float32), 'object_mask': ((n,), torch.bool), 'surface_mask': ((n,), torch.bool),
            'uv': ((n, 2), torch.float32), 'points': ((n, 3), torch.float32), 'normal': ((n, 3), torch.float32),
            'visibility': ((L, n), torch.float32), 'vis_train_gt': ((V, n), torch.float32), 'sampling_idx': ((n,), torch.int64),
            'light_direction': ((L, 3), torch.float32)}
    field = {'object_mask': 'object_mask_out', 'surface_mask': 'surface_mask_out', 'points': 'points_out', 'normal': 'normal_out',
             'visibility': 'visibility_out', 'sampling_idx': 'sampling_idx_out', 'light_direction': 'light_direction_out'}
    for k, t in out.items():
        shape, dt = want[k]
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() == int(torch.Size(shape).numel()), (k, tuple(t.shape), shape)
        setattr(b, field.get(k, k), t.data_ptr())
    _check(_lib.psn_view_batch(ctypes.addressof(b), _stream()), 'view_batch')
    return out


def gather_rows(specs, dense_grads, idx, n_pixels, n_surf, inv=None):
    """Adjoint of scatter_rows for the given dense gradients (contiguous [B, N, C]) -> list of [B*Ns, C] tensors.  inv (the
    pixel -> row map of the scatter): rows of a padded index list that are not the first of their pixel receive zeros."""
    out = [torch.empty(B * n_surf, C, device=idx.device, dtype=torch.float32) for B, C, _ in specs]
    for c0 in range(0, len(specs), SCATTER_MAX_ITEMS):
        n = min(SCATTER_MAX_ITEMS, len(specs) - c0)
        arr = (PsnScatterItem * n)()
        for i in range(n):
            (B, C, _), g, e = specs[c0 + i], dense_grads[c0 + i], arr[i]
            assert g.is_contiguous() and g.shape == (B, n_pixels, C)
            e.rows, e.dense, e.B, e.C = out[c0 + i].data_ptr(), _tptr(g, 'dense_grad'), B, C
        assert idx.dtype == torch.int64 and idx.is_contiguous()
        if inv is not None:
            assert inv.dtype == torch.int32 and inv.is_contiguous() and inv.numel() == n_pixels
            _check(_lib.psn_gather_rows_valid(n, ctypes.addressof(arr), idx.data_ptr(), inv.data_ptr(), n_pixels, n_surf, _stream()),
                   'gather_rows_valid')
            continue
        _check(_lib.psn_gather_rows(n, ctypes.addressof(arr), idx.data_ptr(), n_pixels, n_surf, _stream()), 'gather_rows')
    return out


def secant_step(occ, tau, d_pred, d_low, d_high, f_low, f_high, origin, direction, p_mid):
    """One regula-falsi iteration in place (csrc/sample.hip); occ=None: initial step."""
    _check(_lib.psn_secant_step(_tptr(occ, 'occ', allow_none=True), float(tau), _tptr(d_pred, 'd_pred'), _tptr(d_low, 'd_low'),
                                _tptr(d_high, 'd_high'), _tptr(f_low, 'f_low'), _tptr(f_high, 'f_high'),
                                _tptr(origin, 'origin', allow_none=True), _tptr(direction, 'direction', allow_none=True), _tptr(p_mid, 'p_mid', allow_none=True),
                                d_pred.numel(), _stream()), 'secant_step')


def first_crossing(occ, far, u, omu, near, tau):
    """occ [N, M] sweep occupancies -> (bracket [4, N] float32, flags [N] int32) -- see psn_first_crossing."""
    N, M = occ.shape
    bracket = torch.empty(4, N, device=occ.device, dtype=torch.float32)
    flags = torch.empty(N, device=occ.device, dtype=torch.int32)
    _check(_lib.psn_first_crossing(_tptr(occ, 'occ'), _tptr(far, 'far'), _tptr(u, 'u'), _tptr(omu, 'omu'), float(near), float(tau),
                                   N, M, bracket.data_ptr(), flags.data_ptr(), _stream()), 'first_crossing')
    return bracket, flags


def stage2_loss_fwd(rgb, rgb_gt, alb, alb_j, wgt, wgt_j, vis, vis_gt, nrm, nrm_gt, nrm_j, mask_a, mask_b, l2, inv_denom, weight,
                    count_dev=None):
    """Seven floats on the device: the six loss terms and their weighted total (psn_stage2_loss_fwd)."""
    N = mask_a.numel()
    out = torch.empty(7, device=mask_a.device, dtype=torch.float32)
    partial = workspace(2048 * 6, mask_a.device)
    f = lambda t: _tptr(t, 'loss tensor', allow_none=True)
    b = lambda t: _tptr(t, 'mask', torch.bool)
    _check(_lib.psn_stage2_loss_fwd(f(rgb), f(rgb_gt), 0 if rgb is None else rgb.shape[0], f(alb), f(alb_j), f(wgt), f(wgt_j),
                                    0 if wgt is None else wgt.shape[-1], f(vis), f(vis_gt), 0 if vis is None else vis.shape[0],
                                    f(nrm), f(nrm_gt), f(nrm_j), b(mask_a), b(mask_b), N, int(l2),
                                    ctypes.cast((ctypes.c_float * 6)(*[float(x) for x in inv_denom]), ctypes.c_void_p),
                                    ctypes.cast((ctypes.c_float * 6)(*[float(x) for x in weight]), ctypes.c_void_p),
                                    _tptr(count_dev, 'count_dev', allow_none=True), partial.data_ptr(), out.data_ptr(), _stream()), 'stage2_loss_fwd')
    return out


def stage2_loss_bwd(g_total, rgb, rgb_gt, k_rgb, alb, alb_j, k_alb, wgt, wgt_j, k_wgt, vis, vis_gt, k_vis, nrm, nrm_gt, nrm_j, k_nrm,
                    k_nrmj, mask_a, mask_b, l2, need, count_dev=None):
    """Gradients of the weighted total with respect to the tensors named in ``need`` (a set of 'rgb', 'alb', 'wgt', 'vis',
    'nrm'); returns dict name -> gradient (alb / wgt / nrm also give the jitter gradients as name + '_j')."""
    N = mask_a.numel()
    new = lambda t: torch.empty_like(t)
    d = {}
    if 'rgb' in need: d['rgb'] = new(rgb)
    if 'alb' in need: d['alb'], d['alb_j'] = new(alb), new(alb_j)
    if 'wgt' in need: d['wgt'], d['wgt_j'] = new(wgt), new(wgt_j)
    if 'vis' in need: d['vis'] = new(vis)
    if 'nrm' in need:
        d['nrm'] = new(nrm)
        if nrm_j is not None:
            d['nrm_j'] = new(nrm_j)
    g = lambda k: None if k not in d else d[k].data_ptr()
    f = lambda t: _tptr(t, 'loss tensor', allow_none=True)
    b = lambda t: _tptr(t, 'mask', torch.bool)
    _check(_lib.psn_stage2_loss_bwd(_tptr(g_total, 'g_total'), f(rgb), f(rgb_gt), 0 if rgb is None else rgb.shape[0], float(k_rgb), g('rgb'),
                                    f(alb), f(alb_j), float(k_alb), g('alb'), g('alb_j'), f(wgt), f(wgt_j),
                                    0 if wgt is None else wgt.shape[-1], float(k_wgt), g('wgt'), g('wgt_j'), f(vis), f(vis_gt),
                                    0 if vis is None else vis.shape[0], float(k_vis), g('vis'), f(nrm), f(nrm_gt), f(nrm_j),
                                    float(k_nrm), float(k_nrmj), g('nrm'), g('nrm_j'), b(mask_a), b(mask_b), N, int(l2),
                                    _tptr(count_dev, 'count_dev', allow_none=True), _stream()), 'stage2_loss_bwd')
    return d


def pair_sums(x, V, Ns):
    """x [V * Ns, C] (light-major rows) -> (sum over V [Ns, C], sum over Ns [V, C]) in one pass over x (psn_pair_sums)."""
    C = x.shape[1]
    sx = torch.empty(Ns, C, device=x.device, dtype=torch.float32)
    part = torch.empty(2048, V, C, device=x.device, dtype=torch.float32)
    n_chunks = ctypes.c_int(0)
    _check(_lib.psn_pair_sums(_tptr(x, 'x'), V, Ns, C, sx.data_ptr(), part.data_ptr(), ctypes.byref(n_chunks), _stream()), 'pair_sums')
    return sx, part[:n_chunks.value].sum(0)


def pair_sums_group(xs, V, Ns, pe_l, n_pe, want_bias):
    """xs: list of d z [V * Ns, C] (light-major rows) of the layers that read the input block [table(x_n) | table(l_v)]; pe_l [V, >= n_pe]
    the light table.  -> [(sx [Ns, C], dWl [C, 64] with the first n_pe columns written, bias [C] or None)] in two launches
    (psn_pair_sums_group)."""
    C = xs[0].shape[1]
    dev = xs[0].device
    assert 1 <= len(xs) <= PAIR_GROUP_MAX and all(x.shape == (V * Ns, C) and x.is_contiguous() for x in xs) and pe_l.stride(1) == 1 and pe_l.shape[0] == V
    ws = workspace(int(_lib.psn_pair_sums_group_workspace(len(xs), V, Ns, C)), dev)
    arr = (PsnPairSumsItem * len(xs))()
    out = []
    for e, x, wb in zip(arr, xs, want_bias):
        sx = torch.empty(Ns, C, device=dev, dtype=torch.float32)
        dWl = torch.empty(C, 64, device=dev, dtype=torch.float32)  # (columns >= n_pe are never read)
        b = torch.empty(C, device=dev, dtype=torch.float32) if wb else None
        e.x, e.sx, e.dWl, e.bias = _tptr(x, 'x'), sx.data_ptr(), dWl.data_ptr(), None if b is None else b.data_ptr()
        out.append((sx, dWl, b))
    _check(_lib.psn_pair_sums_group(len(xs), ctypes.addressof(arr), V, Ns, C, _tptr(pe_l, 'pe_l'), pe_l.stride(0), int(n_pe), 64,
                                    ws.data_ptr(), _stream()), 'pair_sums_group')
    return out


def row_adam(items, idx, step_sizes_dev=None):
    """items: list of (param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, step_size) with dense [rows, cols] fp32 device
    tensors; idx: int64 device tensor of the rows that move (psn_row_adam).  step_sizes_dev: fp32 device tensor [len(items)]
    the kernel reads the step sizes from instead (psn_row_adam_dev: graph replay)."""
    arr = (PsnRowAdamItem * len(items))()
    for e, (p, g, m, v, b1, b2, eps, ss) in zip(arr, items):
        p2 = p.view(p.shape[0], -1)
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = _tptr(p, 'param'), _tptr(g, 'grad'), _tptr(m, 'exp_avg'), _tptr(v, 'exp_avg_sq')
        e.rows, e.cols, e.one_minus_beta1, e.one_minus_beta2, e.eps, e.step_size = p2.shape[0], p2.shape[1], 1 - b1, 1 - b2, eps, ss
    assert idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous()
    if step_sizes_dev is not None:
        assert step_sizes_dev.is_cuda and step_sizes_dev.dtype == torch.float32 and step_sizes_dev.numel() >= len(items)
        _check(_lib.psn_row_adam_dev(len(items), ctypes.addressof(arr), idx.data_ptr(), idx.numel(), step_sizes_dev.data_ptr(),
                                     _stream()), 'row_adam_dev')
        return
    _check(_lib.psn_row_adam(len(items), ctypes.addressof(arr), idx.data_ptr(), idx.numel(), _stream()), 'row_adam')


def normalize_rows_fwd(x, eps=1e-12, out=None):
    """F.normalize(x, dim=-1) for [n, 3] rows in one launch."""
    assert x.dim() == 2 and x.shape[1] == 3 and x.is_contiguous()
    y = torch.empty_like(x) if out is None else _out(out, x.shape, x, 'normalize_rows_fwd')
    _check(_lib.psn_normalize_rows_fwd(_tptr(x, 'x'), x.shape[0], float(eps), y.data_ptr(), _stream()), 'normalize_rows_fwd')
    return y


def normalize_rows_bwd(x, g, eps=1e-12, out=None):
    assert x.shape == g.shape and x.shape[1] == 3 and x.is_contiguous() and g.is_contiguous()
    dx = torch.empty_like(x) if out is None else _out(out, x.shape, x, 'normalize_rows_bwd')
    _check(_lib.psn_normalize_rows_bwd(_tptr(x, 'x'), _tptr(g, 'g'), x.shape[0], float(eps), dx.data_ptr(), _stream()), 'normalize_rows_bwd')
    return dx


def light_rows_fwd(dir_table, int_table, idx, eps=1e-12, out=None):
    """(normalize(dir_table[idx]) [L, 3], int_table[idx] [L, 1] or None) in one launch (stage2/trainer.py:376-379).
    out: (d [L, 3], it [L, 1] or None) to write into; an empty index list gives empty outputs without a launch."""
    L = idx.shape[0]
    assert dir_table.dim() == 2 and dir_table.shape[1] == 3 and dir_table.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous()
    d = _out(None if out is None else out[0], (L, 3), dir_table, 'light_rows_fwd')
    it = None
    if int_table is not None:
        assert int_table.shape == (dir_table.shape[0], 1) and int_table.is_contiguous()
        it = _out(None if out is None else out[1], (L, 1), dir_table, 'light_rows_fwd')
    if L == 0:
        return d, it
    _check(_lib.psn_light_rows_fwd(_tptr(dir_table, 'dir_table'), _tptr(int_table, 'int_table', allow_none=True), _tptr(idx, 'idx', torch.int64), L, float(eps),
                                   d.data_ptr(), None if it is None else it.data_ptr(), _stream()), 'light_rows_fwd')
    return d, it


def light_rows_bwd(dir_table, idx, g_dir, g_int, eps=1e-12, out=None):
    """Dense table gradients ([n, 3] or None, [n, 1] or None) of light_rows_fwd, one launch, no separate zero fill (an empty
    index list still launches: the kernel writes the zeros).  out: (dd, di) to write into."""
    n = dir_table.shape[0]
    dd = _out(None if out is None else out[0], (n, 3), dir_table, 'light_rows_bwd') if g_dir is not None else None
    di = _out(None if out is None else out[1], (n, 1), dir_table, 'light_rows_bwd') if g_int is not None else None
    for t in (g_dir, g_int):
        assert t is None or t.is_contiguous()
    for t in (g_dir, g_int):
        assert t is None or t.shape[0] == idx.shape[0]
    ept = lambda t, name, dt=torch.float32: None if t is None else (_tptr(t, name, dt) if t.numel() else _eptr(t, dir_table))
    _check(_lib.psn_light_rows_bwd(_tptr(dir_table, 'dir_table'), ept(idx, 'idx', torch.int64), idx.shape[0], n, float(eps),
                                   ept(g_dir, 'g_dir'), ept(g_int, 'g_int'), None if dd is None else dd.data_ptr(), None if di is None else di.data_ptr(),
                                   _stream()), 'light_rows_bwd')
    return dd, di


def camera_rays(uv, pose, intrinsics, idx=None, scale=1.0, out=None):
    """Normalised camera rays (rend_util.py:90-147, 4 x 4 pose) of the pixels idx (all when None) -> [n, 3], times scale."""
    assert uv.dim() == 3 and uv.shape[0] == 1 and uv.shape[2] == 2 and uv.is_contiguous()
    assert pose.shape == (1, 4, 4) and intrinsics.shape[0] == 1 and intrinsics.shape[1:] == (4, 4) and pose.is_contiguous() and intrinsics.is_contiguous()
    n = uv.shape[1] if idx is None else idx.shape[0]
    out = _out(out, (n, 3), uv, 'camera_rays')
    _check(_lib.psn_camera_rays(_tptr(uv, 'uv'), _tptr(pose, 'pose'), _tptr(intrinsics, 'intrinsics'),
                                _tptr(idx, 'idx', torch.int64, allow_none=True), n, float(scale),
                                out.data_ptr(), _stream()), 'camera_rays')
    return out


def _w4(weights):
    return ctypes.cast((ctypes.c_float * 4)(*[float(x) for x in weights]), ctypes.c_void_p)


def stage1_loss_fwd(rgb, rgb_gt, diff, hit, normal, normal_gt, norm_mask, acc, mask_gt, mask_valid, n_rays, weights, finish=True):
    """(sums [8], terms [5] or None) of psn_stage1_loss_fwd; ``finish=False`` stops after the sums (data parallelism: the
    caller all-reduces sums[4:7] and calls stage1_loss_terms)."""
    N = rgb.shape[0]
    dev = rgb.device
    sums = torch.empty(8, device=dev, dtype=torch.float32)
    terms = torch.empty(5, device=dev, dtype=torch.float32) if finish else None
    partial = workspace(_lib.psn_stage1_loss_partial_floats(), dev)
    f = lambda t: _tptr(t, 'loss tensor', allow_none=True)
    b = lambda t: _tptr(t, 'mask', torch.bool, allow_none=True)
    _check(_lib.psn_stage1_loss_fwd(_tptr(rgb, 'rgb'), _tptr(rgb_gt, 'rgb_gt'), f(diff), b(hit), f(normal),
                                    f(normal_gt), b(norm_mask), f(acc), f(mask_gt),
                                    b(mask_valid), N, int(n_rays), _w4(weights), partial.data_ptr(),
                                    sums.data_ptr(), None if terms is None else terms.data_ptr(), _stream()), 'stage1_loss_fwd')
    return sums, terms


def stage1_loss_terms(sums, n_rays, weights, has_grad, has_norm, has_mask):
    terms = torch.empty(5, device=sums.device, dtype=torch.float32)
    _check(_lib.psn_stage1_loss_terms(_tptr(sums, 'sums'), int(n_rays), _w4(weights), int(has_grad), int(has_norm), int(has_mask),
                                      terms.data_ptr(), _stream()), 'stage1_loss_terms')
    return terms


def stage1_loss_bwd(g_loss, sums, rgb, rgb_gt, hit, normal, normal_gt, norm_mask, acc, mask_gt, mask_valid, n_rays, weights, need):
    """Gradients named in ``need`` (subset of 'rgb', 'diff', 'normal', 'acc') -> dict."""
    N = rgb.shape[0]
    dev = rgb.device
    d = {}
    if 'rgb' in need: d['rgb'] = torch.empty_like(rgb)
    if 'diff' in need: d['diff'] = torch.empty(N, device=dev, dtype=torch.float32)
    if 'normal' in need: d['normal'] = torch.empty_like(normal)
    if 'acc' in need: d['acc'] = torch.empty_like(acc)
    g = lambda k: None if k not in d else d[k].data_ptr()
    b = lambda t: _tptr(t, 'mask', torch.bool, allow_none=True)
    f = lambda t: _tptr(t, 'loss tensor', allow_none=True)
    _check(_lib.psn_stage1_loss_bwd(_tptr(g_loss, 'g_loss'), _tptr(sums, 'sums'), _tptr(rgb, 'rgb'), _tptr(rgb_gt, 'rgb_gt'), b(hit), f(normal),
                                    f(normal_gt), b(norm_mask), f(acc), f(mask_gt), b(mask_valid), N, int(n_rays), _w4(weights),
                                    g('rgb'), g('diff'), g('normal'), g('acc'), _stream()), 'stage1_loss_bwd')
    return d


def surface_normals_fwd(g, hit, eps=1e-5):
    """(norm_pred [N, 3], diff [N]) from g [2 N, 3] and the hit flags [N] bool (psn_surface_normals_fwd)."""
    N = hit.shape[0]
    assert g.shape == (2 * N, 3)
    norm_pred = torch.empty(N, 3, device=g.device, dtype=torch.float32)
    diff = torch.empty(N, device=g.device, dtype=torch.float32)
    _check(_lib.psn_surface_normals_fwd(_tptr(g, 'g'), _tptr(hit, 'hit', torch.bool), N, float(eps), norm_pred.data_ptr(), diff.data_ptr(), _stream()),
           'surface_normals_fwd')
    return norm_pred, diff


def surface_normals_bwd(g, hit, d_norm_pred, d_diff, eps=1e-5):
    N = hit.shape[0]
    dg = torch.empty_like(g)
    _check(_lib.psn_surface_normals_bwd(_tptr(g, 'g'), _tptr(hit, 'hit', torch.bool), N, float(eps), _tptr(d_norm_pred, 'd_norm_pred', allow_none=True),
                                        _tptr(d_diff, 'd_diff', allow_none=True), dg.data_ptr(), _stream()), 'surface_normals_bwd')
    return dg


def stage1_rays(pix, camera_mat, world_mat, radius):
    """Camera origins [n, 3], normalised ray directions [n, 3] and sphere exit depths [n] of the pixels pix [n, 2]
    (stage1/model/common.py:205-226, rendering.py:576-596), one launch; camera_mat [3|4, 3|4], world_mat [4, 4] on the device."""
    assert pix.dim() == 2 and pix.shape[1] == 2 and world_mat.shape == (4, 4) and camera_mat.shape in ((3, 3), (4, 4))
    assert world_mat.is_contiguous() and camera_mat.is_contiguous()
    n = pix.shape[0]
    cam, rays = (torch.empty(n, 3, device=pix.device, dtype=torch.float32) for _ in range(2))
    far = torch.empty(n, device=pix.device, dtype=torch.float32)
    _check(_lib.psn_stage1_rays(_tptr(pix, 'pix'), _tptr(camera_mat, 'camera_mat'), camera_mat.shape[0], _tptr(world_mat, 'world_mat'),
                                float(radius ** 2), n, cam.data_ptr(), rays.data_ptr(), far.data_ptr(), _stream()), 'stage1_rays')
    return cam, rays, far


def surface_points(d_pred, flags, cam, rays, want_d=False):
    """(dists [n], obj_mask [n] bool, points [n, 3][, d_i [n]]) from the root finder's depths and the crossing flags
    (stage1/model/rendering.py:516-522, 84-108), one launch."""
    n = d_pred.shape[0]
    assert flags.dtype == torch.int32 and flags.shape == (n,) and flags.is_contiguous() and cam.shape == (n, 3) and rays.shape == (n, 3)
    dev = d_pred.device
    dists = torch.empty(n, device=dev, dtype=torch.float32)
    obj = torch.empty(n, device=dev, dtype=torch.bool)
    pts = torch.empty(n, 3, device=dev, dtype=torch.float32)
    d_i = torch.empty(n, device=dev, dtype=torch.float32) if want_d else None
    _check(_lib.psn_surface_points(_tptr(d_pred, 'd_pred'), flags.data_ptr(), _tptr(cam, 'cam'), _tptr(rays, 'rays'), n,
                                   None if d_i is None else d_i.data_ptr(), dists.data_ptr(), obj.data_ptr(), pts.data_ptr(),
                                   _stream()), 'surface_points')
    return (dists, obj, pts, d_i) if want_d else (dists, obj, pts)


def stage1_targets(pix, img, mask=None, mask_valid=None, normal=None, norm_mask=None, world_mat=None, cos_thresh=None,
                   want_normal=False):
    """Ground truth of the sampled pixels pix [n, 2] (stage1/model/common.py:172-202, training.py:166-191), one launch:
    (rgb_gt [n, 3], mask_gt [n] float, mask_valid [n] bool, norm_mask_gt [n] bool or None, normal_gt [n, 3] or None)."""
    n = pix.shape[0]
    assert pix.dim() == 2 and pix.shape[1] == 2 and img.dim() == 3 and img.shape[0] == 3
    h, w = int(img.shape[1]), int(img.shape[2])
    for t in (mask, mask_valid, norm_mask):
        assert t is None or tuple(t.shape) == (h, w)
    assert normal is None or tuple(normal.shape) == (3, h, w)
    dev = pix.device
    rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
    mask_gt = torch.empty(n, device=dev, dtype=torch.float32)
    valid = torch.empty(n, device=dev, dtype=torch.bool)
    nmask = torch.empty(n, device=dev, dtype=torch.bool) if norm_mask is not None else None
    ngt = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_normal else None
    _check(_lib.psn_stage1_targets(_tptr(pix, 'pix'), n, h, w, _tptr(img, 'img'), _tptr(mask, 'mask', allow_none=True),
                                   _tptr(mask_valid, 'mask_valid', allow_none=True),
                                   _tptr(normal, 'normal', allow_none=True) if want_normal else None, _tptr(norm_mask, 'norm_mask', allow_none=True),
                                   _tptr(world_mat, 'world_mat', allow_none=True) if want_normal else None, int(cos_thresh is not None),
                                   float(cos_thresh if cos_thresh is not None else 0.0), rgb.data_ptr(), mask_gt.data_ptr(), valid.data_ptr(),
                                   None if ngt is None else ngt.data_ptr(), None if nmask is None else nmask.data_ptr(), _stream()),
           'stage1_targets')
    return rgb, mask_gt, valid, nmask, ngt


def adam_flat(param, grad, exp_avg, exp_avg_sq, segs, beta1, beta2, eps, scalars_dev=None):
    """segs: [(offset, grad_offset, n, neg_step_size, bias_correction2_sqrt)] ranges of the flat buffers (psn_adam_flat);
    more than ADAM_MAX_SEGS ranges go out in several launches.  scalars_dev: fp32 device tensor [len(segs), 2] that the
    kernel reads (neg_step_size, bias_correction2_sqrt) of every range from instead (psn_adam_flat_dev: graph replay)."""
    if scalars_dev is not None:
        assert scalars_dev.is_cuda and scalars_dev.dtype == torch.float32 and scalars_dev.is_contiguous() and scalars_dev.numel() >= 2 * len(segs)
    for t in (param, grad, exp_avg, exp_avg_sq):
        assert t.dim() == 1 and t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
    assert exp_avg.numel() == exp_avg_sq.numel() == param.numel()
    for s0 in range(0, len(segs), ADAM_MAX_SEGS):
        part = segs[s0:s0 + ADAM_MAX_SEGS]
        arr = (PsnAdamSeg * len(part))()
        for a, (off, goff, n, ns, bc) in zip(arr, part):
            assert 0 <= off and off + n <= param.numel() and 0 <= goff and goff + n <= grad.numel()
            a.offset, a.grad_offset, a.n, a.neg_step_size, a.bias_correction2_sqrt = int(off), int(goff), int(n), float(ns), float(bc)
        if scalars_dev is not None:
            _check(_lib.psn_adam_flat_dev(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), len(part), arr,
                                          float(1 - beta1), float(beta2), float(1 - beta2), float(eps),
                                          scalars_dev.data_ptr() + 8 * s0, _stream()), 'adam_flat_dev')
            continue
        _check(_lib.psn_adam_flat(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), len(part), arr,
                                  float(1 - beta1), float(beta2), float(1 - beta2), float(eps), _stream()), 'adam_flat')


def shadow_points(surf, ldir, n_steps, lnear, lfar, u, omu, box):
    """In-box shadow-ray sample points (psn_shadow_points) -> (pts [cap,3], rows [cap] int64, counter [1] int64 on the
    device: the number of valid leading entries).  cap = all L*Ns*n_steps rows (worst case)."""
    L, Ns = ldir.shape[0], surf.shape[0]
    cap = L * Ns * n_steps
    pts = torch.empty(max(cap, 1), 3, device=surf.device, dtype=torch.float32)
    rows = torch.empty(max(cap, 1), device=surf.device, dtype=torch.int64)
    counter = torch.zeros(1, device=surf.device, dtype=torch.int64)
    _check(_lib.psn_shadow_points(_tptr(surf, 'surf'), _tptr(ldir, 'ldir'), Ns, L, int(n_steps), float(lnear), float(lfar),
                                  _tptr(u, 'u'), _tptr(omu, 'omu'), float(box), pts.data_ptr(), rows.data_ptr(), counter.data_ptr(),
                                  _stream()), 'shadow_points')
    return pts, rows, counter


def _last_path(path):
    """Fill ``path`` (a PsnMlpPath, or None) with what this thread's last launch of the fused MLP engine ran (psn_mlp_last_path)."""
    if path is not None:
        _check(_lib.psn_mlp_last_path(ctypes.byref(path)), 'mlp_last_path')


def mlp_infer_pe(desc, packed_w, packed_b, points, pe_octaves, pe_scale, out=None, macs_per_row=None, n_rows_dev=None, out_rows=None, path=None):
    """Network on gamma(pe_scale * points) with the encoding formed inside the kernel (psn_mlp_infer_pe) -> [Q, n_out].
    ``n_rows_dev`` (int64 [1] on the device): only the first n_rows_dev[0] points are valid (psn_mlp_infer_pe_indirect; the
    grid covers all Q); ``out_rows`` (int64 [Q]): row r is written to out[out_rows[r]] -- ``out`` is then required.
    ``path``: a PsnMlpPath that receives what the library launched."""
    Q = points.shape[0]
    assert points.shape == (Q, 3) and points.is_contiguous()
    indirect = n_rows_dev is not None
    if out is None:
        assert out_rows is None, 'a scatter needs its destination'
        out = torch.empty(Q, desc.n_out, device=points.device, dtype=torch.float32)
    assert out.is_contiguous() and (out_rows is not None or out.numel() == Q * desc.n_out)
    if Q == 0:
        return out
    if indirect:
        assert n_rows_dev.dtype == torch.int64 and n_rows_dev.is_cuda and n_rows_dev.numel() == 1
        assert out_rows is None or (out_rows.dtype == torch.int64 and out_rows.is_cuda and out_rows.is_contiguous() and out_rows.numel() >= Q)
        # (no flop count for the profile: how many rows were evaluated is known to the device only)
        with _Prof('mlp_infer', Q, None):
            _check(_lib.psn_mlp_infer_pe_indirect(ctypes.byref(desc), _tptr(packed_w, 'packed_w'), _tptr(packed_b, 'packed_b'),
                                                  _tptr(points, 'points'), Q, n_rows_dev.data_ptr(),
                                                  None if out_rows is None else out_rows.data_ptr(), int(pe_octaves), float(pe_scale),
                                                  out.data_ptr(), _stream()), 'mlp_infer_pe_indirect')
        _last_path(path)
        return out
    assert out_rows is None
    with _Prof('mlp_infer', Q, None if macs_per_row is None else 2.0 * macs_per_row * Q):
        _check(_lib.psn_mlp_infer_pe(ctypes.byref(desc), _tptr(packed_w, 'packed_w'), _tptr(packed_b, 'packed_b'), _tptr(points, 'points'),
                                     Q, int(pe_octaves), float(pe_scale), out.data_ptr(), _stream()), 'mlp_infer_pe')
    _last_path(path)
    return out


def march_sweep(desc, packed_w, packed_b, origin, direction, far, u, omu, near, n_steps, tau, pe_octaves, pe_scale,
                early_exit=True, macs_per_row=None, path=None):
    """Occupancy of the n_steps sweep points of every ray (psn_march_sweep) -> (occ [N, n_steps], skip flags [N] int32 or None).
    early_exit: blocks of 64 steps behind a ray's first sign change are not evaluated (their occ entries are uninitialised).
    path: a PsnMlpPath that receives what the library launched."""
    N = origin.shape[0]
    assert origin.shape == (N, 3) and direction.shape == (N, 3) and far.shape == (N,) and u.numel() == n_steps == omu.numel()
    occ = torch.empty(N, n_steps, device=origin.device, dtype=torch.float32)
    skip = torch.zeros(N, device=origin.device, dtype=torch.int32) if early_exit else None
    if N == 0:
        return occ, skip
    Q = N * n_steps
    # measurement runs (PROFILE_EVENTS set) count the 64-step blocks that were really evaluated: the event carries the device
    # counter and the flops of ONE block, so that the reader prices evaluated work, not the N x M rows of the dense sweep
    count = torch.zeros(1, device=origin.device, dtype=torch.int64) if PROFILE_EVENTS is not None else None
    with _Prof('march_sweep', Q, None if (macs_per_row is None or count is None) else (count, 2.0 * macs_per_row * 64)):
        _check(_lib.psn_march_sweep(ctypes.byref(desc), _tptr(packed_w, 'packed_w'), _tptr(packed_b, 'packed_b'), _tptr(origin, 'origin'),
                                    _tptr(direction, 'direction'), _tptr(far, 'far'), _tptr(u, 'u'), _tptr(omu, 'omu'), float(near), N,
                                    int(n_steps), float(tau), int(pe_octaves), float(pe_scale),
                                    None if skip is None else skip.data_ptr(), None if count is None else count.data_ptr(),
                                    occ.data_ptr(), _stream()), 'march_sweep')
    _last_path(path)
    return occ, skip


def root_find(desc, packed_w, packed_b, origin, direction, bracket, tau, n_iter, pe_octaves, pe_scale, out=None, path=None):
    """n_iter secant iterations on every ray in one launch (psn_root_find) -> d_pred [N].
    ``out``: the caller's [N] destination; ``path``: a PsnMlpPath that receives what the library launched."""
    N = origin.shape[0]
    assert bracket.shape == (4, N)
    if out is None:
        out = torch.empty(N, device=origin.device, dtype=torch.float32)
    assert out.is_contiguous() and out.numel() == N
    if N == 0:  # (empty tensors have no device pointer to hand over) nothing is launched: a zeroed path
        if path is not None:
            ctypes.memset(ctypes.byref(path), 0, ctypes.sizeof(path))
        return out
    with _Prof('root_find', N, None):
        _check(_lib.psn_root_find(ctypes.byref(desc), _tptr(packed_w, 'packed_w'), _tptr(packed_b, 'packed_b'), _tptr(origin, 'origin'),
                                  _tptr(direction, 'direction'), _tptr(bracket, 'bracket'), N, float(tau), int(n_iter), int(pe_octaves),
                                  float(pe_scale), _tptr(out, 'd_pred'), _stream()), 'root_find')
    _last_path(path)
    return out


def workspace(n_floats, device):
    """Scratch buffer per (device, stream), grown on demand: launches on one stream are ordered, so they may share it;
    two streams (the small stage-2 networks run beside the visibility launch on a side stream) must not.  A buffer that a
    HIP-graph capture has used (``capturing(True)`` ... ``capturing(False)`` around the capture: stage2/graph.py) is never
    freed when a larger one replaces it -- the captured launches hold its address."""
    di = device.index if device.index is not None else torch._C._cuda_getDevice()
    key = (di, torch._C._cuda_getCurrentRawStream(di))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < n_floats:
        if buf is not None and key in _ws_pinned:
            _ws_retired.append(buf)
            _ws_pinned.discard(key)
        buf = torch.empty(max(n_floats, 1 << 22), device=device, dtype=torch.float32)
        _ws_cache[key] = buf
    if _ws_capturing[0]:
        _ws_pinned.add(key)
    return buf


_ws_capturing = [False]
_ws_pinned = set()
_ws_retired = []


def capturing(on):
    """Tell the binding that the launches issued from now on are being captured into a HIP graph (or no longer are)."""
    _ws_capturing[0] = bool(on)


def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, 'matrix operand must be row-major with unit column stride'
    return t.stride(0)


def _mat_ptr(t, name):
    """2-D row-major view (may be a column slice of a wider buffer: ld = stride(0), so no contiguity rule)."""
    return _tptr(t, name, contiguous=False)


def gemm(A, B, trans_a=False, trans_b=False, bias=None, epi=EPI_NONE, aux_in=None, out=None, aux_out=None,
         split_k=1, aux_in2=None, colsum_a=None):
    """out[M,N] = epi(op(A) @ op(B)).  A/B/out/aux may be row-major views with a row stride.
    colsum_a (trans_a only): [M] tensor that receives the column sums of A (= the bias gradient when A = dZ)."""
    if trans_a:
        K, M = A.shape
    else:
        M, K = A.shape
    if trans_b:
        N, Kb = B.shape
    else:
        Kb, N = B.shape
    assert K == Kb, 'gemm: inner dimensions differ (%d vs %d)' % (K, Kb)
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    assert out.shape == (M, N)
    ws = None
    if split_k > 1:
        ws = workspace(split_k * M * (N + 1), A.device)
    _check(_lib.psn_gemm(int(trans_a), int(trans_b), M, N, K, _mat_ptr(A, 'A'), _ld(A), _mat_ptr(B, 'B'), _ld(B),
                         _mat_ptr(out, 'out'), _ld(out), _tptr(bias, 'bias', allow_none=True), epi,
                         None if aux_in is None else _mat_ptr(aux_in, 'aux_in'), 0 if aux_in is None else _ld(aux_in),
                         None if aux_in2 is None else _mat_ptr(aux_in2, 'aux_in2'),
                         0 if aux_in2 is None else _ld(aux_in2),
                         None if aux_out is None else _mat_ptr(aux_out, 'aux_out'),
                         0 if aux_out is None else _ld(aux_out), split_k,
                         None if ws is None else ws.data_ptr(), _tptr(colsum_a, 'colsum_a', allow_none=True), _stream()), 'gemm')
    return out


def _tn_aligned(t):
    return t is None or (t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(0) >= 4)


def _tn_is_big(it):
    """Products that psn_gemm_tn_grouped sends to its one-256x256-tile-per-workgroup kernel."""
    return (not it.get('b_div') and not it.get('b_mod') and 128 < it['A'].shape[1] <= 256 and 128 < it['B'].shape[1] <= 256
            and _tn_aligned(it['A']) and _tn_aligned(it['B']) and _tn_aligned(it.get('A2')) and _tn_aligned(it.get('B2')))


def _tn_is_tall(it):
    """Products that psn_gemm_tn_grouped sends to its 256 x (<= 64)-tile kernel (input-block gradients)."""
    return (not it.get('b_div') and not it.get('b_mod') and 128 < it['A'].shape[1] <= 256 and it['B'].shape[1] <= 64
            and it.get('B_tab2') is None
            and _tn_aligned(it['A']) and _tn_aligned(it['B']) and _tn_aligned(it.get('A2')) and _tn_aligned(it.get('B2')))


# EXPERIMENT (BASELINE configs[4] bf16 path): the 256 x 256-tile weight gradients on the bf16 matrix pipe with split operands
# (psn_gemm_tn_grouped_x3).  Process-wide switch for A/B runs and the labelled bench objects; never on by default.
WGRAD_X3 = False


class wgrad_precision(object):
    """``with hip.wgrad_precision(mode):`` -- the 256 x 256-tile weight-gradient products issued inside take
    'fp32'   the exact kernel (v_mfma_f32_32x32x2_f32);
    'bf16x6' the split-bf16 kernel with three pieces per operand and six partial products (fp32-class results);
    'bf16x3' two pieces, three partial products (~16 significant bits);
    'bf16'   plain bf16 operands, fp32 accumulation.
    Wrap the BACKWARD pass (that is where the products are issued)."""
    PRODUCTS = {'bf16x6': 6, 'bf16x3': 3, 'bf16': 1}

    def __init__(self, mode):
        assert mode in ('fp32', 'bf16x6', 'bf16x3', 'bf16'), mode
        self.mode = mode

    def __enter__(self):
        global WGRAD_X3
        self.saved, WGRAD_X3 = WGRAD_X3, self.mode != 'fp32'
        self.saved_products = _lib.psn_gemm_tn_x3_set_products(self.PRODUCTS.get(self.mode, 6))
        return self

    def __exit__(self, *exc):
        global WGRAD_X3
        WGRAD_X3 = self.saved
        _lib.psn_gemm_tn_x3_set_products(self.saved_products)
        return False


def _tn_shape(it, K):
    """(M, N) of the result of one item of gemm_tn_grouped, after the shape rules of its operands."""
    A, B = it['A'], it['B']
    if it.get('b_div') or it.get('b_mod'):  # B is a table: row k of the product reads B[(k // b_div) % b_mod]
        assert A.shape[0] == K and int(it.get('b_mod') or B.shape[0]) <= B.shape[0] and it.get('A2') is None
    else:
        # a product may cover a row PREFIX of the pass (operands with fewer rows than items[0]): k_rows
        assert A.shape[0] == B.shape[0] <= K, 'gemm_tn_grouped: a product has at most the K rows of the first one'
    M, N = A.shape[1], B.shape[1]
    Bt2 = it.get('B_tab2')
    if Bt2 is not None:  # second table side by side: columns N .. N + Bt2.shape[1] - 1 of the virtual operand
        assert N % 4 == 0 and int(it.get('b2_div', 0)) > 0
        N += Bt2.shape[1]
    return M, N


def _tn_fill(e, it, K, ptr):
    """The operand fields of one PsnGemmTnItem (everything but C and colsum_a); ptr(tensor, name) -> address."""
    A, B = it['A'], it['B']
    M, N = _tn_shape(it, K)
    b_div, b_mod = int(it.get('b_div', 0)), int(it.get('b_mod', 0))
    if b_div or b_mod:
        b_div, b_mod = max(b_div, 1), (b_mod if b_mod else B.shape[0])
    Bt2 = it.get('B_tab2')
    A2, B2 = it.get('A2'), it.get('B2')
    e.A, e.lda, e.B, e.ldb = ptr(A, 'A'), _ld(A), ptr(B, 'B'), _ld(B)
    if A2 is not None:
        assert A2.shape == A.shape and B2.shape == B.shape
        e.A2, e.lda2, e.B2, e.ldb2 = ptr(A2, 'A2'), _ld(A2), ptr(B2, 'B2'), _ld(B2)
    e.M, e.N = M, N
    e.accumulate = int(bool(it.get('accumulate')))
    e.b_div, e.b_mod = b_div, b_mod
    if Bt2 is not None:
        e.B_tab2, e.ldb_tab2 = ptr(Bt2, 'B_tab2'), _ld(Bt2)
        e.b2_div, e.b2_mod, e.b_split = int(it['b2_div']), int(it.get('b2_mod', Bt2.shape[0])), B.shape[1]
    e.k_rows = 0 if A.shape[0] == K else A.shape[0]


def _addr(t):
    return 0 if t is None else t.data_ptr()


def gemm_plan(A, B, out, trans_a=False, trans_b=False, aux_in=None, aux_in2=None, aux_out=None, split_k=1, workspace_addr=0):
    """What ``gemm`` would launch for operands placed like these: a host-only query (psn_gemm_plan), so the tensors may live
    on any device -- only their shapes, row strides and the low bits of their addresses are looked at."""
    K, M = A.shape if trans_a else A.shape[::-1]
    N = B.shape[0] if trans_b else B.shape[1]
    pl = PsnGemmPlan()  # noqa: F821
    ld = lambda t: 0 if t is None else _ld(t)
    _check(_lib.psn_gemm_plan(M, N, K, _addr(A), _ld(A), _addr(B), _ld(B), _addr(out), _ld(out), _addr(aux_in), ld(aux_in),
                              _addr(aux_in2), ld(aux_in2), _addr(aux_out), ld(aux_out), split_k, workspace_addr,
                              ctypes.addressof(pl)), 'gemm_plan')
    return pl


def gemm_tn_plan(items, split_k, workspace_addr=0):
    """What one launch of ``gemm_tn_grouped`` would run for these items (at most GEMM_TN_MAX_ITEMS, explicit split_k): a
    host-only query (psn_gemm_tn_plan); tensors on any device, 'out' required."""
    K = items[0]['A'].shape[0]
    arr = (PsnGemmTnItem * len(items))()  # noqa: F821
    for e, it in zip(arr, items):
        _tn_fill(e, it, K, lambda t, name: t.data_ptr())
        e.C, e.ldc = it['out'].data_ptr(), _ld(it['out'])
        e.colsum_a = 16 if it.get('colsum') else None
    pl = PsnGemmTnPlan()  # noqa: F821
    _check(_lib.psn_gemm_tn_plan(len(items), ctypes.addressof(arr), K, split_k, workspace_addr, ctypes.addressof(pl)), 'gemm_tn_plan')
    return pl


def colsum_plan(X, n_w=0, workspace_addr=0):
    """What ``colsum`` would launch for an X placed like this one (host-only, psn_colsum_plan)."""
    pl = PsnColsumPlan()  # noqa: F821
    _check(_lib.psn_colsum_plan(_addr(X), n_w, X.shape[0], X.shape[1], _ld(X), workspace_addr, ctypes.addressof(pl)), 'colsum_plan')
    return pl


def gemm_tn_grouped(items, split_k=None, x3=None):
    """Weight gradients of one backward pass in one launch.  items: list of dicts with A [K,M], B [K,N] (row-major
    views, row stride allowed), optional A2 / B2 (second product summed into the same result), optional out [M,N]
    (+ accumulate=True) and colsum (True -> the column sums of A are returned too).  Returns [(C, colsum or None)].
    split_k = K slices per product of the 128 x 128-tile path (default: enough (tile, slice) work items to cover the
    256 CUs about four times with K chunks of at least 512 rows); the 256 x 256-tile path picks its own."""
    res = []
    K = items[0]['A'].shape[0]
    dev = items[0]['A'].device
    # which kernel of psn_gemm_tn_grouped a product goes to: decided ONCE per item (the predicates were evaluated four times each)
    kinds = {id(it): ('big' if _tn_is_big(it) else ('tall' if _tn_is_tall(it) else 'tile')) for it in items}
    if split_k is None:
        work = 0
        for it in items:
            if kinds[id(it)] == 'tile':
                tiles = ((it['A'].shape[1] + 127) // 128) * ((it['B'].shape[1] + 127) // 128)
                work += tiles * (2 if it.get('A2') is not None else 1)
        want = max(1, (1024 + work - 1) // max(work, 1))
        # K chunks of at least 512 rows -- for a SHORT product (the 128- / 64-wide BRDF / normal networks of a 4096-pixel rank
        # shard: K = 7k rows, 5 - 6 tiles) that bound left 84 workgroups of 33 k-steps each on 256 CUs, 100 us per call that
        # nothing else filled; there a chunk may shrink to 128 rows (8 k-steps): 340 workgroups, the reduction is 20 MB
        min_rows = 512 if K >= 16384 else 128
        split_k = int(max(1, min(want, K // min_rows if K >= min_rows else 1, 256)))
    for c0 in range(0, len(items), GEMM_TN_MAX_ITEMS):
        chunk = items[c0:c0 + GEMM_TN_MAX_ITEMS]
        arr = (PsnGemmTnItem * len(chunk))()
        need = 0
        keep = []
        # slices per product of the one-tile-per-workgroup path (mirrors psn_gemm_tn_grouped, which re-checks the size)
        is_big = lambda it_: kinds[id(it_)] == 'big'
        n_big = sum((2 if it.get('A2') is not None else 1) for it in chunk if is_big(it))
        split_big = 1
        if n_big:
            want = max(1, min(256 // n_big, K // 256 if K >= 256 else 1))
            kc = -(-K // want)
            kc = (kc + 15) // 16 * 16  # (the kernel rounds its K chunk to 32-row k-tiles: never more slices than this bound)
            split_big = -(-K // kc)
        n_tall = sum((2 if it.get('A2') is not None else 1) for it in chunk if kinds[id(it)] == 'tall')
        split_tall = 1
        if n_tall:
            want = max(1, min(256 // n_tall, K // 256 if K >= 256 else 1))
            kc = -(-K // want)
            kc = (kc + 15) // 16 * 16
            split_tall = -(-K // kc)
        for i, it in enumerate(chunk):
            M, N = _tn_shape(it, K)
            C = it.get('out')
            if C is None:
                C = torch.empty(M, N, device=dev, dtype=torch.float32)
            assert C.shape == (M, N)
            cs = torch.empty(M, device=dev, dtype=torch.float32) if it.get('colsum') else None
            A2 = it.get('A2')
            e = arr[i]
            _tn_fill(e, it, K, _mat_ptr)
            e.C, e.ldc = _mat_ptr(C, 'out'), _ld(C)
            e.colsum_a = None if cs is None else cs.data_ptr()
            sk = max(split_k, split_big) if is_big(it) else (max(split_k, split_tall) if kinds[id(it)] == 'tall' else split_k)
            need += (2 if A2 is not None else 1) * sk * M * N + sk * M + 16
            keep.append((C, cs))
        ws = workspace(need, dev)
        flops = sum(2.0 * (arr[i].k_rows or K) * arr[i].M * arr[i].N * (2 if chunk[i].get('A2') is not None else 1) for i in range(len(chunk)))
        use_x3 = WGRAD_X3 if x3 is None else bool(x3)
        with _Prof('gemm_tn_grouped', flops):
            _check((_lib.psn_gemm_tn_grouped_x3 if use_x3 else _lib.psn_gemm_tn_grouped)(
                len(chunk), ctypes.addressof(arr), K, split_k, ws.data_ptr(), ws.numel(), _stream()), 'gemm_tn_grouped')
        res += keep
    return res


def colsum(X, out=None, accumulate=False, row_weight=None):
    """Plain column sums [N]: out[n] (+)= sum_m X[m, n]; or with row_weight [M, n_w <= 4] (a 1-D [M] counts as one
    column) the small weight gradient [n_w, N]: out[j, n] (+)= sum_m w[m, j] X[m, n]."""
    M, N = X.shape
    n_w, ldw, wp = 0, 0, None
    if row_weight is not None:
        w2 = row_weight if row_weight.dim() == 2 else row_weight.reshape(M, 1)  # (reshape(0, -1) is ambiguous: M may be 0)
        assert w2.stride(1) == 1 and 1 <= w2.shape[1] <= 4
        n_w, ldw, wp = w2.shape[1], w2.stride(0), _mat_ptr(w2, 'row_weight')
    if out is None:
        out = torch.empty((n_w, N) if n_w else (N,), device=X.device, dtype=torch.float32)
    ws = workspace(2048 * N, X.device)
    xp = _mat_ptr(X, 'X')
    if M == 0:  # an empty tensor has no address: the workspace stands in for the operands, of which no row is read
        xp, wp = ws.data_ptr(), (ws.data_ptr() if n_w else None)
    _check(_lib.psn_colsum(xp, wp, n_w, ldw, M, N, _ld(X), out.data_ptr(), int(accumulate), ws.data_ptr(),
                           _stream()), 'colsum')
    return out


# --------------------------------------------------------------------------- fused MLP inference
def mlp_pack_layer(W, n_mt, k_tiles, dst, transpose=False):
    """W: 2-D fp32 device matrix (row-major view, unit column stride); with transpose=True its transpose is packed.
    Zero-extended to [n_mt*32, k_tiles*32] and written to dst (flat float view) in stage order."""
    assert W.dim() == 2 and W.stride(1) == 1 and W.is_cuda and W.dtype == torch.float32
    rows, cols = (W.shape[1], W.shape[0]) if transpose else (W.shape[0], W.shape[1])
    _check(_lib.psn_mlp_pack_layer(W.data_ptr(), W.stride(0), rows, cols, int(transpose), n_mt, k_tiles, dst.data_ptr(),
                                   _stream()), 'mlp_pack_layer')


def mlp_pack_layers(plan):
    """plan: list of (W, transpose, n_mt, k_tiles, dst[, format = W_F32]) like mlp_pack_layer, packed in ONE launch per 24 blocks."""
    for c0 in range(0, len(plan), PACK_MAX_ITEMS):
        chunk = plan[c0:c0 + PACK_MAX_ITEMS]
        arr = (PsnPackItem * len(chunk))()
        for e, item in zip(arr, chunk):
            W, transpose, n_mt, k_tiles, dst = item[:5]
            e.format = item[5] if len(item) > 5 else W_F32
            assert W.dim() == 2 and W.stride(1) == 1 and W.is_cuda and W.dtype == torch.float32
            assert dst.is_contiguous() and dst.numel() == n_mt * k_tiles * 1024
            rows, cols = (W.shape[1], W.shape[0]) if transpose else (W.shape[0], W.shape[1])
            e.W, e.dst, e.ldw = W.data_ptr(), dst.data_ptr(), W.stride(0)
            e.rows, e.cols, e.transpose, e.n_mt, e.k_tiles = rows, cols, int(transpose), n_mt, k_tiles
        _check(_lib.psn_mlp_pack_layers(len(chunk), ctypes.addressof(arr), _stream()), 'mlp_pack_layers')


class block_order(object):
    """``with hip.block_order('row'):`` -- the lean engine's (group, point) row sets in row order instead of the default
    point-tile-major order (psn_mlp_block_order; results are bit-identical, the order only decides what stays in L2)."""

    def __init__(self, order):
        assert order in ('point', 'row'), order
        self.order = order

    def __enter__(self):
        self.saved = _lib.psn_mlp_block_order(1 if self.order == 'point' else 0)
        return self

    def __exit__(self, *exc):
        _lib.psn_mlp_block_order(self.saved)
        return False


def mlp_infer(desc, packed_w, packed_b, tab_a, a_div, a_mod, tab_b, b_div, b_mod, n_rows, out=None, init_a=None,
              init_b=None, save=None, save_row0=0, mask=None, aux2=None, save2=None, act_init=None, macs_per_row=None,
              rank_init=None, save_tiles=None, save2_tiles=None, act_init_rows=None, live=None, save_bits=None, path=None):
    """One launch of the fused engine (psn_mlp_launch; the library decides between the lean and the chain engine).
    save: list (one entry per hidden layer, None allowed) of [n_rows - save_row0, 256] tensors that receive the
    post-activation outputs of the rows >= save_row0.
    rank_init = (coef [n_rows, k], basis [k, init_stride]), k <= 4: rank-k init of the layers with init_off >= 0.
    act_init [act_init_rows (default n_rows), width]: initial activations; the rows behind them start from zeros.
    live = (count float32 [1] on the device, period): the rows [0, save_row0) are groups of `period` rows of which the first
    count[0] are real (PsnMlpLaunch.live_count; plain forward launches only): all-padding workgroups write zeros and leave.
    save_bits: list like ``save`` of int64 [n_rows - save_row0, 4] tensors (or None) that receive the sign bits of the dumped
    activations (PsnMlpLaunch.save_bits_ptrs); a chain layer with ACT_RELU_BITS takes such a tensor as its ``mask`` entry.
    path: a PsnMlpPath that receives what the library launched."""
    o, keep = PsnMlpLaunch(), []     # (keep: the host arrays of the launch, alive until it returns)
    if save_tiles is not None or save2_tiles is not None:  # per layer: bit mt = the 16-column tile mt of the dump is written
        tiles_arr = (ctypes.c_uint32 * (2 * MAX_LAYERS))(*([0xFFFFFFFF] * (2 * MAX_LAYERS)))
        for base, lst in ((0, save_tiles), (MAX_LAYERS, save2_tiles)):
            for l, m in enumerate(lst or []):
                if m is not None:
                    tiles_arr[base + l] = int(m)
        keep.append(tiles_arr)
        o.dump_tiles = ctypes.addressof(tiles_arr)
    if rank_init is not None:
        rk_coef, rk_basis = rank_init
        o.rk_k = rk_k = rk_basis.shape[0]
        assert rk_coef.shape == (n_rows, rk_k) and rk_coef.is_contiguous() and rk_basis.is_contiguous() and 1 <= rk_k <= 4
        assert rk_basis.shape[1] == desc.init_stride, 'rank_init: the basis rows are init_stride floats'
        o.rk_coef, o.rk_basis = _tptr(rk_coef, 'rk_coef'), _tptr(rk_basis, 'rk_basis')
    if act_init is not None:
        o.act_init_rows = n_rows if act_init_rows is None else act_init_rows
        assert act_init.is_contiguous() and act_init.shape[0] >= o.act_init_rows, 'act_init: fewer rows than act_init_rows'
        o.act_init = _tptr(act_init, 'act_init')
    if out is None and desc.n_out > 0:
        out = torch.empty(n_rows, desc.n_out, device=packed_w.device, dtype=torch.float32)
    n_hidden = desc.n_layers - 1 if desc.n_out > 0 else desc.n_layers

    def ptr_array(lst, n, name, words=None):
        """HOST array of the device pointers of ``lst``; words: the entries are sign-bit words (None: those that are int64)."""
        if lst is None:
            return None
        assert len(lst) == n, '%s: expected %d entries' % (name, n)
        is_words = lambda t: t.dtype == torch.int64 if words is None else words
        keep.append((ctypes.c_void_p * n)(*[None if t is None else (_bits_ptr(t, name) if is_words(t) else _tptr(t, name)) for t in lst]))
        return ctypes.addressof(keep[-1])

    o.mask_ptrs, o.aux2_ptrs, o.save2_ptrs = (ptr_array(lst, desc.n_layers, name) for lst, name in ((mask, 'mask'), (aux2, 'aux2'), (save2, 'save2')))
    o.save_ptrs, o.save_bits_ptrs = ptr_array(save, n_hidden, 'save', False), ptr_array(save_bits, n_hidden, 'save_bits', True)
    for t, b in zip(save or [], save_bits or []):
        assert b is None or (t is not None and b.shape == (t.shape[0], 4))
    if live is not None:
        cnt, period = live
        assert cnt.is_cuda and cnt.dtype == torch.float32 and cnt.numel() == 1 and int(period) >= 1
        o.live_count, o.live_period = cnt.data_ptr(), int(period)
    o.tab_a, o.a_div, o.a_mod = _tptr(tab_a, 'tab_a', allow_none=True), a_div, a_mod
    o.tab_b, o.b_div, o.b_mod = _tptr(tab_b, 'tab_b', allow_none=True), b_div, b_mod
    o.init_a, o.init_b = _tptr(init_a, 'init_a', allow_none=True), _tptr(init_b, 'init_b', allow_none=True)
    o.save_row0, o.n_rows, o.out = save_row0, n_rows, _tptr(out, 'out', allow_none=True)
    path = PsnMlpPath() if path is None else path
    with _Prof('mlp_infer', n_rows, None if macs_per_row is None else 2.0 * macs_per_row * n_rows) as prof:
        _check(_lib.psn_mlp_launch(ctypes.byref(desc), _tptr(packed_w, 'packed_w'), _tptr(packed_b, 'packed_b'), ctypes.byref(o),
                                   ctypes.byref(path), _stream()), 'mlp_infer')
        prof.name = 'mlp_chain' if path.chain else 'mlp_infer'     # the lean / the chain engine, as the library chose
    return out


# --------------------------------------------------------------------------- weight normalisation
def weight_norm_fwd(vs, gs, scales, out=None):
    """[v_l * (g_l / |v_l|_row) * scale_l] for all layers in one launch (<= 16 per launch); out: the list of w_l to write into."""
    out = [torch.empty_like(v) for v in vs] if out is None else [_out(o, v.shape, v, 'weight_norm_fwd') for o, v in zip(out, vs)]
    assert len(out) == len(vs) == len(gs)
    for c0 in range(0, len(vs), WN_MAX_ITEMS):
        n = min(WN_MAX_ITEMS, len(vs) - c0)
        arr = (PsnWnItem * n)()
        for i in range(n):
            v, g = vs[c0 + i], gs[c0 + i]
            assert v.dim() == 2 and g.numel() == v.shape[0]
            e = arr[i]
            e.v, e.g, e.w = _tptr(v, 'weight_v'), _tptr(g, 'weight_g'), out[c0 + i].data_ptr()
            e.rows, e.cols, e.scale = v.shape[0], v.shape[1], float(scales[c0 + i])
        _check(_lib.psn_weight_norm_fwd(n, ctypes.addressof(arr), _stream()), 'weight_norm_fwd')
    return out


def weight_norm_bwd(vs, gs, scales, dws, out=None):
    """(dv_l, dg_l) of weight_norm_fwd for the output gradients dws (dense, same shapes as vs); out: (dvs, dgs) to write into."""
    dvs = [torch.empty_like(v) for v in vs] if out is None else [_out(o, v.shape, v, 'weight_norm_bwd') for o, v in zip(out[0], vs)]
    dgs = [torch.empty_like(g) for g in gs] if out is None else [_out(o, g.shape, g, 'weight_norm_bwd') for o, g in zip(out[1], gs)]
    assert len(dvs) == len(dgs) == len(vs) == len(gs) == len(dws)
    for c0 in range(0, len(vs), WN_MAX_ITEMS):
        n = min(WN_MAX_ITEMS, len(vs) - c0)
        arr = (PsnWnItem * n)()
        for i in range(n):
            v, g = vs[c0 + i], gs[c0 + i]
            e = arr[i]
            e.v, e.g, e.dw = _tptr(v, 'weight_v'), _tptr(g, 'weight_g'), _tptr(dws[c0 + i], 'dw')
            e.dv, e.dg = dvs[c0 + i].data_ptr(), dgs[c0 + i].data_ptr()
            e.rows, e.cols, e.scale = v.shape[0], v.shape[1], float(scales[c0 + i])
        _check(_lib.psn_weight_norm_bwd(n, ctypes.addressof(arr), _stream()), 'weight_norm_bwd')
    return dvs, dgs


# --------------------------------------------------------------------------- bf16 inference engine (evaluation only)
def lowp_pack(W, permuted, n_ot, ks0, n_ks, dst, planes=1):
    """k-steps [ks0, ks0 + n_ks) of the fp32 matrix W (row-major view) -> dst (flat bfloat16 view, n_ks * n_ot * planes * 512
    elements) in fragment order (psn_lowp_pack): planes = 1 for the bf16 engine, 3 (hi / mid / lo of every weight) for the split one."""
    assert W.dim() == 2 and W.stride(1) == 1 and W.is_cuda and W.dtype == torch.float32
    assert dst.dtype == torch.bfloat16 and dst.is_contiguous() and dst.numel() == n_ks * n_ot * planes * 512
    _check(_lib.psn_lowp_pack(W.data_ptr(), W.stride(0), W.shape[0], W.shape[1], int(permuted), n_ot, ks0, n_ks, planes,
                              dst.data_ptr(), _stream()), 'lowp_pack')


def lowp_pack_bias(V, pieces, dst=None):
    """V [n, 256] fp32 -> [n, 4096] bfloat16 bias k-steps (psn_lowp_pack_bias): K slots 0 .. pieces - 1 = the value's leading bf16
    pieces; 2 for the bf16 engine (one row per (group, input layer)), 3 for the split one."""
    assert V.is_cuda and V.dtype == torch.float32 and V.is_contiguous() and V.dim() == 2 and V.shape[1] == 256
    if dst is None:
        dst = torch.empty(V.shape[0], 4096, device=V.device, dtype=torch.bfloat16)
    assert dst.dtype == torch.bfloat16 and dst.is_contiguous() and dst.numel() == V.shape[0] * 4096
    _check(_lib.psn_lowp_pack_bias(V.data_ptr(), V.shape[0], pieces, dst.data_ptr(), _stream()), 'lowp_pack_bias')
    return dst


def _bf16_stream(t, name):
    """Device pointer of a packed weight or bias stream."""
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
        raise RuntimeError('%s: must be a contiguous bfloat16 HIP tensor' % name)
    return t.data_ptr()


def _n_in(desc):
    """Hidden layers of a PsnBf16Desc that read the input block."""
    return sum(1 for l in range(desc.n_hidden) if desc.has_in[l])


def _bf16_table(t, name):
    """Device pointer of an input table of the bf16 engine ([n, 64] bfloat16, contiguous), or None."""
    if t is not None and (t.dim() != 2 or t.shape[1] != 64):
        raise RuntimeError('%s: must be a contiguous [n, 64] bfloat16 HIP tensor' % name)
    return _tptr(t, name, torch.bfloat16, allow_none=True)


def mlp_infer_bf16(desc, packed_w, final_bias, tab_a, a_div, a_mod, tab_b, b_div, b_mod, n_rows, out=None):
    if out is None:
        out = torch.empty(n_rows, desc.n_out, device=packed_w.device, dtype=torch.float32)
    assert packed_w.dtype == torch.bfloat16 and packed_w.is_cuda and packed_w.is_contiguous()
    assert final_bias.numel() == 32
    ptrs = (_tptr(final_bias, 'final_bias'), _bf16_table(tab_a, 'tab_a'), _bf16_table(tab_b, 'tab_b'), _tptr(out, 'out'))
    if n_rows == 0:  # validated like any launch; nothing to launch (an empty tensor has no device pointer to hand over)
        return out
    with _Prof('mlp_infer_bf16', n_rows):
        _check(_lib.psn_mlp_infer_bf16(ctypes.byref(desc), packed_w.data_ptr(), ptrs[0], ptrs[1], a_div, a_mod, ptrs[2], b_div, b_mod,
                                       n_rows, ptrs[3], _stream()), 'mlp_infer_bf16')
    return out


def mlp_infer_bf16_grouped(desc, packed_w, final_bias, tab_a, group_bias, n_groups, out=None):
    """Rows (g, n) -> g * tab_a.shape[0] + n; group_bias [n_groups * n_in_layers, 4096] bfloat16 (lowp_pack_bias, 2 pieces)."""
    rows = tab_a.shape[0]
    if out is None:
        out = torch.empty(n_groups * rows, desc.n_out, device=packed_w.device, dtype=torch.float32)
    assert packed_w.dtype == torch.bfloat16 and packed_w.is_cuda and packed_w.is_contiguous()
    assert final_bias.numel() == 32
    n_in = _n_in(desc)
    if not (group_bias.is_cuda and group_bias.dtype == torch.bfloat16 and group_bias.is_contiguous()
            and group_bias.numel() == n_groups * n_in * 4096):
        raise RuntimeError('group_bias: must be a contiguous [n_groups * %d, 4096] bfloat16 HIP tensor' % n_in)
    assert out.numel() == n_groups * rows * desc.n_out
    ptrs = (_tptr(final_bias, 'final_bias'), _bf16_table(tab_a, 'tab_a'), _tptr(out, 'out'))
    if n_groups * rows == 0:
        return out
    with _Prof('mlp_infer_bf16', n_groups * rows):
        _check(_lib.psn_mlp_infer_bf16_grouped(ctypes.byref(desc), packed_w.data_ptr(), ptrs[0], ptrs[1], rows, group_bias.data_ptr(), n_groups,
                                               ptrs[2], _stream()), 'mlp_infer_bf16_grouped')
    return out


# --------------------------------------------------------------------------- split-bf16 ("bf16x6") engine, experiment
X3_KS = 8 * 3 * 512  # bf16 elements of one hidden-layer k-step: 8 output tiles x 3 planes x 1 KB


def mlp_infer_x3_grouped(desc, packed_w, bias_steps, final_bias, U, V, out=None, macs_per_row=None):
    """Rows (g, n) -> g * U.shape[0] + n on the split-bf16 engine (psn_mlp_infer_x3_grouped); U [Ns, n_in * 256], V [G, n_in * 256]
    fp32 init tables of the layers that read the input block."""
    rows, n_groups = U.shape[0], V.shape[0]
    if out is None:
        out = torch.empty(n_groups * rows, desc.n_out, device=packed_w.device, dtype=torch.float32)
    n_in = _n_in(desc)
    streams = (_bf16_stream(packed_w, 'packed_w'), _bf16_stream(bias_steps, 'bias_steps'))
    assert U.shape[1] == V.shape[1] == n_in * 256 and bias_steps.numel() == desc.n_hidden * 4096
    assert final_bias.numel() == 32 and out.numel() == n_groups * rows * desc.n_out
    ptrs = (_tptr(final_bias, 'final_bias'), _tptr(U, 'U'), _tptr(V, 'V'), _tptr(out, 'out'))
    if n_groups * rows == 0:
        return out
    with _Prof('mlp_infer_x3', n_groups * rows, None if macs_per_row is None else 2.0 * macs_per_row * n_groups * rows):
        _check(_lib.psn_mlp_infer_x3_grouped(ctypes.byref(desc), streams[0], streams[1], ptrs[0],
                                             ptrs[1], rows, ptrs[2], n_groups, ptrs[3], _stream()), 'mlp_infer_x3_grouped')
    return out


def mlp_infer_x3_occ(desc, packed_w, bias_steps, final_bias, points, pe_octaves, pe_scale, skip_layer, pe_first, out=None,
                     n_rows_dev=None, out_rows=None, macs_per_row=None):
    """sigmoid(-10 logit) of the stage-1 occupancy network for [Q, 3] points on the split-bf16 engine (psn_mlp_infer_x3_occ):
    the encoding is formed in the kernel, the activation is softplus(beta = 100).  n_rows_dev / out_rows as hip.mlp_infer_pe."""
    Q = points.shape[0]
    assert points.dim() == 2 and points.shape[1] == 3
    if out is None:
        assert out_rows is None
        out = torch.empty(Q, desc.n_out, device=points.device, dtype=torch.float32)
    streams = (_bf16_stream(packed_w, 'packed_w'), _bf16_stream(bias_steps, 'bias_steps'))
    assert bias_steps.numel() == desc.n_hidden * 4096 and final_bias.numel() == 32 and desc.n_out == 1
    if n_rows_dev is not None:
        assert n_rows_dev.is_cuda and n_rows_dev.dtype == torch.int64 and n_rows_dev.numel() == 1
    if out_rows is not None:
        assert out_rows.is_cuda and out_rows.dtype == torch.int64 and out_rows.is_contiguous() and out_rows.numel() >= Q
    ptrs = (_tptr(final_bias, 'final_bias'), _tptr(points, 'points'), _tptr(out, 'out'))
    if Q == 0:
        return out
    with _Prof('mlp_infer_x3_occ', Q, None if macs_per_row is None else 2.0 * macs_per_row * Q):
        _check(_lib.psn_mlp_infer_x3_occ(ctypes.byref(desc), streams[0], streams[1], ptrs[0],
                                         ptrs[1], Q, None if n_rows_dev is None else n_rows_dev.data_ptr(),
                                         None if out_rows is None else out_rows.data_ptr(), int(pe_octaves), float(pe_scale),
                                         int(skip_layer), int(pe_first), ptrs[2], _stream()), 'mlp_infer_x3_occ')
    return out


# --------------------------------------------------------------------------- SG shading
def sg_shade_fwd(light_dir, view, normal, albedo, weights, lobe, light_int, light_int_scalar, vis, specular_rgb):
    L, Ns, nb = light_dir.shape[0], view.shape[0], lobe.shape[0]
    rgb = torch.empty(L * Ns, 3, device=view.device, dtype=torch.float32)
    spec = torch.empty(L * Ns, 3 if specular_rgb else 1, device=view.device, dtype=torch.float32)
    if Ns == 0:  # no points: nothing to launch (an empty tensor has no device pointer to hand over)
        return rgb, spec
    _check(_lib.psn_sg_shade_fwd(_tptr(light_dir, 'light_dir'), _tptr(view, 'view'), _tptr(normal, 'normal'),
                                 _tptr(albedo, 'albedo'), _tptr(weights, 'weights'), _tptr(lobe, 'lobe'),
                                 _tptr(light_int, 'light_int', allow_none=True),
                                 1 if light_int is None or light_int.dim() == 1 else light_int.shape[1],
                                 float(light_int_scalar), _tptr(vis, 'vis', allow_none=True),
                                 L, Ns, nb, int(bool(specular_rgb)), _tptr(rgb, 'rgb'), _tptr(spec, 'spec'), _stream()),
           'sg_shade_fwd')
    return rgb, spec


def sg_shade_bwd(light_dir, view, normal, albedo, weights, lobe, light_int, light_int_scalar, vis, specular_rgb,
                 g_rgb, g_spec, want_vis):
    L, Ns, nb = light_dir.shape[0], view.shape[0], lobe.shape[0]
    dev = view.device
    d_albedo = torch.empty(Ns, 3, device=dev)
    d_weights = torch.empty_like(weights)
    d_normal = torch.empty(Ns, 3, device=dev)
    d_vis = torch.empty(L * Ns, device=dev) if want_vis else None
    d_ldir = torch.empty(L, 3, device=dev)
    d_lint = torch.empty(L, device=dev) if light_int is not None else None
    if Ns == 0:  # the per-light gradients are sums over no points
        return d_albedo, d_weights, d_normal, d_vis, torch.zeros_like(d_ldir), None if d_lint is None else torch.zeros_like(d_lint)
    ws = workspace(((Ns + 63) // 64) * L * 4, dev)
    _check(_lib.psn_sg_shade_bwd(_tptr(light_dir, 'light_dir'), _tptr(view, 'view'), _tptr(normal, 'normal'),
                                 _tptr(albedo, 'albedo'), _tptr(weights, 'weights'), _tptr(lobe, 'lobe'),
                                 _tptr(light_int, 'light_int', allow_none=True), float(light_int_scalar), _tptr(vis, 'vis', allow_none=True),
                                 L, Ns, nb, int(bool(specular_rgb)), _tptr(g_rgb, 'g_rgb'), _tptr(g_spec, 'g_spec', allow_none=True),
                                 _tptr(d_albedo, 'd_albedo'), _tptr(d_weights, 'd_weights'), _tptr(d_normal, 'd_normal'),
                                 _tptr(d_vis, 'd_vis', allow_none=True), _tptr(d_ldir, 'd_ldir'), _tptr(d_lint, 'd_lint', allow_none=True),
                                 ws.data_ptr(), _stream()), 'sg_shade_bwd')
    return d_albedo, d_weights, d_normal, d_vis, d_ldir, d_lint


# --------------------------------------------------------------------------- GGX microfacet shading
def mf_shade_fwd(light_dir, view, normal, albedo, rough, light_int, light_int_scalar, f0, vis):
    L, Ns = light_dir.shape[0], view.shape[0]
    rgb = torch.empty(L * Ns, 3, device=view.device, dtype=torch.float32)
    if Ns == 0:
        return rgb
    _check(_lib.psn_mf_shade_fwd(_tptr(light_dir, 'light_dir'), _tptr(view, 'view'), _tptr(normal, 'normal'),
                                 _tptr(albedo, 'albedo'), _tptr(rough, 'rough'), _tptr(light_int, 'light_int', allow_none=True),
                                 float(light_int_scalar), float(f0), _tptr(vis, 'vis', allow_none=True), L, Ns, _tptr(rgb, 'rgb'),
                                 _stream()), 'mf_shade_fwd')
    return rgb


def mf_shade_bwd(light_dir, view, normal, albedo, rough, light_int, light_int_scalar, f0, vis, g_rgb, want_vis):
    L, Ns = light_dir.shape[0], view.shape[0]
    dev = view.device
    d_albedo = torch.empty(Ns, 3, device=dev)
    d_rough = torch.empty(Ns, device=dev)
    d_normal = torch.empty(Ns, 3, device=dev)
    d_vis = torch.empty(L * Ns, device=dev) if want_vis else None
    d_ldir = torch.empty(L, 3, device=dev)
    d_lint = torch.empty(L, device=dev) if light_int is not None else None
    if Ns == 0:
        return d_albedo, d_rough, d_normal, d_vis, torch.zeros_like(d_ldir), None if d_lint is None else torch.zeros_like(d_lint)
    ws = workspace(((Ns + 63) // 64) * L * 4, dev)
    _check(_lib.psn_mf_shade_bwd(_tptr(light_dir, 'light_dir'), _tptr(view, 'view'), _tptr(normal, 'normal'),
                                 _tptr(albedo, 'albedo'), _tptr(rough, 'rough'), _tptr(light_int, 'light_int', allow_none=True),
                                 float(light_int_scalar), float(f0), _tptr(vis, 'vis', allow_none=True), L, Ns, _tptr(g_rgb, 'g_rgb'),
                                 _tptr(d_albedo, 'd_albedo'), _tptr(d_rough, 'd_rough'), _tptr(d_normal, 'd_normal'),
                                 _tptr(d_vis, 'd_vis', allow_none=True), _tptr(d_ldir, 'd_ldir'), _tptr(d_lint, 'd_lint', allow_none=True),
                                 ws.data_ptr(), _stream()), 'mf_shade_bwd')
    return d_albedo, d_rough, d_normal, d_vis, d_ldir, d_lint


def march_sweep_x3(desc, packed_w, bias_steps, final_bias, origin, direction, far, u, omu, near, n_steps, tau, pe_octaves, pe_scale,
                   skip_layer, pe_first, early_exit=True, macs_per_row=None):
    """hip.march_sweep on the split-bf16 engine (psn_march_sweep_x3; opt-in experiment): occupancy of the n_steps sweep points of
    every ray -> (occ [N, n_steps], skip flags [N] int32 or None); blocks of 128 steps behind a ray's first sign change are not
    evaluated when early_exit (their entries are uninitialised).  n_steps a multiple of 128."""
    N = origin.shape[0]
    assert origin.shape == (N, 3) and direction.shape == (N, 3) and far.shape == (N,) and u.numel() == n_steps == omu.numel()
    streams = (_bf16_stream(packed_w, 'packed_w'), _bf16_stream(bias_steps, 'bias_steps'))
    occ = torch.empty(N, n_steps, device=origin.device, dtype=torch.float32)
    skip = torch.zeros(N, device=origin.device, dtype=torch.int32) if early_exit else None
    if N == 0:
        return occ, skip
    count = torch.zeros(1, device=origin.device, dtype=torch.int64) if PROFILE_EVENTS is not None else None
    with _Prof('march_sweep_x3', N * n_steps, None if (macs_per_row is None or count is None) else (count, 2.0 * macs_per_row * 128)):
        _check(_lib.psn_march_sweep_x3(ctypes.byref(desc), streams[0], streams[1], _tptr(final_bias, 'final_bias'),
                                       _tptr(origin, 'origin'), _tptr(direction, 'direction'), _tptr(far, 'far'), _tptr(u, 'u'), _tptr(omu, 'omu'),
                                       float(near), N, int(n_steps), float(tau), int(pe_octaves), float(pe_scale), int(skip_layer), int(pe_first),
                                       None if skip is None else skip.data_ptr(), occ.data_ptr(), None if count is None else count.data_ptr(),
                                       _stream()), 'march_sweep_x3')
    return occ, skip


# --------------------------------------------------------------------------- stage-1 mesh extraction (csrc/mesh.hip)
def mise_flags(resolution, device):
    """Zeroed flag bytes of a (resolution + 1)^3 grid, padded to whole 4-byte words (psn_mise_collect / psn_mise_refine)."""
    n3 = (resolution + 1) ** 3
    return torch.zeros((n3 + 3) // 4 * 4, dtype=torch.uint8, device=device)


def mise_collect(flags, resolution, box_size, capacity, count):
    """Pending grid points -> (rows int64 [capacity], points float32 [capacity, 3]); count (int64 [1] on the device) receives their
    number; the points become known (psn_mise_collect)."""
    assert flags.numel() == ((resolution + 1) ** 3 + 3) // 4 * 4 and count.numel() == 1
    rows = torch.empty(capacity, dtype=torch.int64, device=flags.device)
    points = torch.empty(capacity, 3, dtype=torch.float32, device=flags.device)
    _check(_lib.psn_mise_collect(_tptr(flags, 'flags', torch.uint8), int(resolution), float(box_size), int(capacity), rows.data_ptr(),
                                 points.data_ptr(), _tptr(count, 'count', torch.int64), _stream()), 'mise_collect')
    return rows, points


def mise_refine(grid, flags, vox, resolution0, depth, threshold, pending):
    """One refinement round in place (psn_mise_refine); pending (int64 [1] on the device) receives the number of new grid points."""
    res = resolution0 << depth
    assert grid.numel() == (res + 1) ** 3 and flags.numel() == ((res + 1) ** 3 + 3) // 4 * 4 and pending.numel() == 1
    assert vox.numel() == sum((resolution0 << l) ** 3 for l in range(depth))
    _check(_lib.psn_mise_refine(_tptr(grid, 'grid'), _tptr(flags, 'flags', torch.uint8), _tptr(vox, 'vox', torch.uint8), int(resolution0),
                                int(depth), float(threshold), _tptr(pending, 'pending', torch.int64), _stream()), 'mise_refine')


def grid_ffill(grid):
    """MISE.to_dense's hole filling, in place on a cubic [n, n, n] grid whose holes are NaN (psn_grid_ffill)."""
    n = grid.shape[0]
    assert grid.shape == (n, n, n)
    with _Prof('grid_ffill', 8 * grid.numel()):
        _check(_lib.psn_grid_ffill(_tptr(grid, 'grid'), n, _stream()), 'grid_ffill')
    return grid


def marching_cubes(grid, threshold, box_size=0.0):
    """Marching cubes over a cubic [n, n, n] grid padded (virtually) with -1e6 (psn_mc_count, psn_mc_emit) ->
    (vertices float64 [V, 3], faces int64 [F, 3]) on the device.  box_size > 0: vertices in world units
    (stage1/model/extracting.py:175-181); otherwise in units of the padded lattice.  One host synchronisation (the two totals)."""
    n = grid.shape[0]
    assert grid.shape == (n, n, n)
    dev = grid.device
    nb = int(_lib.psn_mc_blocks(n))
    if nb == 0:
        raise RuntimeError('marching_cubes: %d points per axis are not supported (2 .. %d)' % (n, MESH_MAX_RESOLUTION + 1))
    n_cells = (n + 1) ** 3
    code = torch.empty(n_cells, dtype=torch.uint8, device=dev)
    blk = torch.empty(2, nb, dtype=torch.int32, device=dev)
    with _Prof('mc_count', 4 * grid.numel()):
        _check(_lib.psn_mc_count(_tptr(grid, 'grid'), n, float(threshold), code.data_ptr(), blk[0].data_ptr(), blk[1].data_ptr(), _stream()),
               'mc_count')
    incl = torch.cumsum(blk, dim=1, dtype=torch.int64)
    base = (incl - blk).contiguous()
    n_v, n_f = (int(x) for x in incl[:, -1].tolist())
    vertices = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
    faces = torch.empty(n_f, 3, dtype=torch.int64, device=dev)
    if n_v == 0:
        return vertices, faces
    v_off = torch.empty(n_cells, dtype=torch.int32, device=dev)
    with _Prof('mc_emit', 24 * n_v + 24 * n_f):
        _check(_lib.psn_mc_emit(_tptr(grid, 'grid'), n, float(threshold), code.data_ptr(), base[0].data_ptr(), base[1].data_ptr(), n_v, n_f,
                                float(box_size), v_off.data_ptr(), vertices.data_ptr(), faces.data_ptr(), _stream()), 'mc_emit')
    return vertices, faces


# --------------------------------------------------------------------------- point-to-mesh distance (csrc/meshdist.hip)
def tri_grid(lo, hi, cell, n, max_span):
    """The host-side descriptor of the triangle grid (PsnTriGrid): bounding box, cell edge, cells per axis, oversize limit."""
    g = PsnTriGrid()
    for a in range(3):
        g.lo[a], g.hi[a], g.n[a] = float(lo[a]), float(hi[a]), int(n[a])
    g.cell, g.max_span = float(cell), int(max_span)
    return g


def _mesh_ptrs(vertices, faces):
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError('mesh: vertices [V, 3] and faces [F, 3] expected, got %s / %s' % (tuple(vertices.shape), tuple(faces.shape)))
    return _tptr(vertices, 'vertices', torch.float64), _tptr(faces, 'faces', torch.int64)


def tri_grid_count(grid, vertices, faces, n_over, out=None):
    """Index build, first pass (psn_tri_grid_count) -> (cell_count int32 [cells], over_list int32 [F]); n_over (int64 [1] on the
    device) receives the length of the oversize list.  ``out``: the two, preallocated (cell_count is zeroed by the call whatever it
    held; of over_list only the first n_over entries are written)."""
    vp, fp = _mesh_ptrs(vertices, faces)
    cells = grid.n[0] * grid.n[1] * grid.n[2]
    assert n_over.numel() == 1
    o = out if out is not None else (None, None)
    cell_count = _out(o[0], (cells,), vertices, 'tri_grid_count: cell_count', torch.int32)
    over_list = _out(o[1], (faces.shape[0],), vertices, 'tri_grid_count: over_list', torch.int32)
    with _Prof('tri_grid_count', 96 * faces.shape[0]):
        _check(_lib.psn_tri_grid_count(ctypes.byref(grid), vp, fp, faces.shape[0], cell_count.data_ptr(), over_list.data_ptr(),
                                       _tptr(n_over, 'n_over', torch.int64), _stream()), 'tri_grid_count')
    return cell_count, over_list


def tri_grid_fill(grid, vertices, faces, cursor, n_entries, out=None):
    """Index build, second pass (psn_tri_grid_fill): cursor (int32 [cells], the exclusive scan of the counts; advanced in place) ->
    list int32 [n_entries]; ``out``: the list, preallocated."""
    vp, fp = _mesh_ptrs(vertices, faces)
    assert cursor.numel() == grid.n[0] * grid.n[1] * grid.n[2]
    lst = _out(out, (int(n_entries),), vertices, 'tri_grid_fill: list', torch.int32)
    with _Prof('tri_grid_fill', 96 * faces.shape[0]):
        _check(_lib.psn_tri_grid_fill(ctypes.byref(grid), vp, fp, faces.shape[0], _tptr(cursor, 'cursor', torch.int32), int(n_entries),
                                      lst.data_ptr(), _stream()), 'tri_grid_fill')
    return lst


def mesh_index(grid, vertices, faces, cell_start, lst, over_list, n_over):
    """The built index as the four queries below take it (PsnMeshIndex): the grid, the mesh, cell_start int32 [cells + 1], the cell
    lists and the first n_over entries of over_list.  Everything about it is checked here, once; the object keeps the tensors whose
    addresses it holds (``tensors``)."""
    ix = PsnMeshIndex()  # noqa: F821
    ix.grid, ix.n_faces, ix.n_over = grid, faces.shape[0], int(n_over)
    ix.vertices, ix.faces = _mesh_ptrs(vertices, faces)
    ix.cell_start, ix.list, ix.over_list = (_tptr(t, name, torch.int32) for name, t in (('cell_start', cell_start), ('list', lst),
                                                                                       ('over_list', over_list)))
    assert cell_start.numel() == grid.n[0] * grid.n[1] * grid.n[2] + 1 and 0 <= n_over <= over_list.numel()
    ix.tensors = (vertices, faces, cell_start, lst, over_list)
    return ix


def closest_point(index, points, order=None, n_tests=None):
    """psn_closest_point: points float64 [Q, 3] -> (closest float64 [Q, 3], distance float64 [Q], triangle id int64 [Q]) over the whole
    mesh; order = the permutation in which the points are worked on (or None); n_tests (int64 [1]) accumulates the number of
    point-triangle tests."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError('closest_point: points [Q, 3] expected, got %s' % (tuple(points.shape),))
    q = points.shape[0]
    assert order is None or order.numel() == q
    dev = points.device
    closest = torch.empty(q, 3, dtype=torch.float64, device=dev)
    dist = torch.empty(q, dtype=torch.float64, device=dev)
    tri = torch.empty(q, dtype=torch.int64, device=dev)
    if q == 0:
        return closest, dist, tri
    with _Prof('closest_point', q):
        _check(_lib.psn_closest_point(ctypes.byref(index), _tptr(points, 'points', torch.float64),
                                      None if order is None else _tptr(order, 'order', torch.int64), q,
                                      closest.data_ptr(), dist.data_ptr(), tri.data_ptr(),
                                      None if n_tests is None else _tptr(n_tests, 'n_tests', torch.int64), _stream()), 'closest_point')
    return closest, dist, tri


# --------------------------------------------------------------------------- ray casting (csrc/meshray.hip)
def ray_cast(index, origins, directions, t_min=0.0, t_max=float('inf'), order=None, any_hit=False, n_tests=None, want_bary=True):
    """psn_ray_cast: origins / directions float64 [Q, 3] -> (t float64 [Q], triangle id int64 [Q], barycentrics float64 [Q, 3] or None,
    hit uint8 [Q]): the first hit with t_min <= t <= t_max over the whole mesh (a miss: inf, -1, NaN, 0), or with ``any_hit`` only
    ``hit``.  order = the permutation in which the rays are worked on (or None); n_tests (int64 [1]) accumulates the number of
    ray-triangle tests."""
    for name, x in (('origins', origins), ('directions', directions)):
        _tptr(x, 'ray_cast: %s' % name, torch.float64)
        if x.dim() != 2 or x.shape[1] != 3:
            raise RuntimeError('ray_cast: %s [Q, 3] expected, got %s' % (name, tuple(x.shape)))
    if origins.shape != directions.shape:
        raise RuntimeError('ray_cast: %d origins and %d directions' % (origins.shape[0], directions.shape[0]))
    q = origins.shape[0]
    assert order is None or order.numel() == q
    dev = origins.device
    t = torch.empty(q, dtype=torch.float64, device=dev)
    tri = torch.empty(q, dtype=torch.int64, device=dev)
    bary = torch.empty(q, 3, dtype=torch.float64, device=dev) if want_bary else None
    hit = torch.empty(q, dtype=torch.uint8, device=dev)
    if q == 0:
        return t, tri, bary, hit
    with _Prof('ray_cast_any' if any_hit else 'ray_cast', q):
        _check(_lib.psn_ray_cast(ctypes.byref(index), origins.data_ptr(), directions.data_ptr(),
                                 None if order is None else _tptr(order, 'order', torch.int64), q, float(t_min), float(t_max),
                                 RAY_ANY_HIT if any_hit else RAY_FIRST_HIT, t.data_ptr(), tri.data_ptr(),  # noqa: F821
                                 None if bary is None else bary.data_ptr(), hit.data_ptr(),
                                 None if n_tests is None else _tptr(n_tests, 'n_tests', torch.int64), _stream()), 'ray_cast')
    return t, tri, bary, hit


# --------------------------------------------------------------------------- occlusion of rows (csrc/meshocclude.hip)
def occlusion_rows(index, points, normals, table, local=True, bias=0.0, t_max=float('inf'), bits=False, n_tests=None, out=None):
    """psn_occlusion_rows: points / normals float64 [R, 3], table float64 [K, 3] -> (hits int32 [R], visible int32 [R], ao float64 [R],
    bent float64 [R, 3], words int32 [R, ceil(K / 32)] or None): per row the K rays of the table (about the normal with ``local``, as
    given and only where they face the normal without) any-hit against the whole mesh.  out: the five outputs to write into (words
    None without ``bits``); n_tests (int64 [1]) accumulates the number of ray-triangle tests."""
    for name, x in (('points', points), ('normals', normals), ('table', table)):
        _tptr(x, 'occlusion_rows: %s' % name, torch.float64)
        if x.dim() != 2 or x.shape[1] != 3:
            raise RuntimeError('occlusion_rows: %s [R, 3] expected, got %s' % (name, tuple(x.shape)))
    if points.shape != normals.shape:
        raise RuntimeError('occlusion_rows: %d points and %d normals' % (points.shape[0], normals.shape[0]))
    r, k = points.shape[0], table.shape[0]
    n_words = (k + 31) // 32
    given = (None,) * 5 if out is None else out
    hits = _out(given[0], (r,), points, 'occlusion_rows: hits', torch.int32)
    visible = _out(given[1], (r,), points, 'occlusion_rows: visible', torch.int32)
    ao = _out(given[2], (r,), points, 'occlusion_rows: ao', torch.float64)
    bent = _out(given[3], (r, 3), points, 'occlusion_rows: bent', torch.float64)
    words = _out(given[4], (r, n_words), points, 'occlusion_rows: words', torch.int32) if bits else None
    with _Prof('occlusion_rows', r * k):
        _check(_lib.psn_occlusion_rows(ctypes.byref(index), _eptr(points, table), _eptr(normals, table), r, _eptr(table, points), k,
                                       OCC_LOCAL if local else OCC_WORLD, float(bias), float(t_max),  # noqa: F821
                                       _eptr(hits, table), _eptr(visible, table), _eptr(ao, table), _eptr(bent, table),
                                       None if words is None else _eptr(words, table),
                                       None if n_tests is None else _tptr(n_tests, 'n_tests', torch.int64), _stream()), 'occlusion_rows')
    return hits, visible, ao, bent, words


# --------------------------------------------------------------------------- the views on surface rows (csrc/meshproject.hip)
def project_rows(index, points, normals, views, images, hw=None, masks=None, bias=0.0, cos_min=0.0, uniform=False, camera_normal=False,
                 bits=False, n_tests=None, out=None):
    """psn_project_rows: points / normals float64 [R, 3], views float64 [V, 16] (hull._views), images uint8 or float32 [V, H, W, C] (or
    None with ``hw`` = (H, W): visibility only, C = 0), masks uint8 [V, H, W] or None -> (sum [R, C], sum_sq [R, C], weight [R], n_seen
    int32 [R], best_view int32 [R], best_value [R, C], words int32 [R, ceil(V / 32)] or None); the three [R, C] outputs are None with
    C = 0.  out: the seven outputs to write into (None where none is made); n_tests (int64 [1]) accumulates the ray-triangle tests."""
    for name, x in (('points', points), ('normals', normals)):
        _tptr(x, 'project_rows: %s' % name, torch.float64)
        if x.dim() != 2 or x.shape[1] != 3:
            raise RuntimeError('project_rows: %s [R, 3] expected, got %s' % (name, tuple(x.shape)))
    if points.shape != normals.shape or normals.device != points.device:
        raise RuntimeError('project_rows: %d points and %d normals (on one device)' % (points.shape[0], normals.shape[0]))
    _tptr(views, 'project_rows: views', torch.float64)
    if views.dim() != 2 or views.shape[1] != 16 or views.device != points.device:
        raise RuntimeError('project_rows: views [V, 16] on the rows\' device expected, got %s' % (tuple(views.shape),))
    r, v = int(points.shape[0]), int(views.shape[0])
    if images is None:
        if hw is None:
            raise RuntimeError('project_rows: without images, hw = (H, W) is required')
        H, W, C, ip, ty = int(hw[0]), int(hw[1]), 0, None, IMG_F32  # noqa: F821
    else:
        ip = _tptr(images, 'project_rows: images', tuple(IMG_TYPES))
        if images.dim() != 4 or images.shape[0] != v or images.device != points.device or images.numel() == 0:
            raise RuntimeError('project_rows: images [%d, H, W, C] on the rows\' device expected, got %s' % (v, tuple(images.shape)))
        H, W, C, ty = int(images.shape[1]), int(images.shape[2]), int(images.shape[3]), IMG_TYPES[images.dtype]
        if hw is not None and (int(hw[0]), int(hw[1])) != (H, W):
            raise RuntimeError('project_rows: hw = %r, the images are %d x %d' % (tuple(hw), H, W))
    mp = None
    if masks is not None:
        mp = _tptr(masks, 'project_rows: masks', torch.uint8)
        if tuple(masks.shape) != (v, H, W) or masks.device != points.device:
            raise RuntimeError('project_rows: masks [%d, %d, %d] on the rows\' device expected, got %s' % (v, H, W, tuple(masks.shape)))
    n_words = (v + 31) // 32
    given = (None,) * 7 if out is None else out
    if C == 0 and any(given[i] is not None for i in (0, 1, 5)):
        raise RuntimeError('project_rows: out holds sum / sum_sq / best_value buffers, but there are no images')
    total = _out(given[0], (r, C), points, 'project_rows: sum', torch.float64) if C else None
    total_sq = _out(given[1], (r, C), points, 'project_rows: sum_sq', torch.float64) if C else None
    weight = _out(given[2], (r,), points, 'project_rows: weight', torch.float64)
    n_seen = _out(given[3], (r,), points, 'project_rows: n_seen', torch.int32)
    best_view = _out(given[4], (r,), points, 'project_rows: best_view', torch.int32)
    best_value = _out(given[5], (r, C), points, 'project_rows: best_value', torch.float64) if C else None
    words = _out(given[6], (r, n_words), points, 'project_rows: words', torch.int32) if bits else None
    opt = lambda t: None if t is None else _eptr(t, views)
    with _Prof('project_rows', r * v):
        _check(_lib.psn_project_rows(ctypes.byref(index), _eptr(points, views), _eptr(normals, views), r, _eptr(views, points), v, ip, ty, H, W, C,
                                     mp, float(bias), float(cos_min),
                                     PROJECT_WEIGHT_UNIFORM if uniform else PROJECT_WEIGHT_COSINE,  # noqa: F821
                                     PROJECT_FRAME_CAMERA_NORMAL if camera_normal else PROJECT_FRAME_RAW,  # noqa: F821
                                     opt(total), opt(total_sq), _eptr(weight, views), _eptr(n_seen, views), _eptr(best_view, views),
                                     opt(best_value), opt(words),
                                     None if n_tests is None else _tptr(n_tests, 'n_tests', torch.int64), _stream()), 'project_rows')
    return total, total_sq, weight, n_seen, best_view, best_value, words


# --------------------------------------------------------------------------- crossing counts (csrc/meshinside.hip)
def mesh_crossings(index, points, axis=2, order=None, want_below=True, want_on=True, n_tests=None):
    """psn_mesh_crossings: points float64 [Q, 3] -> (above int32 [Q], below int32 [Q] or None, on int32 [Q] or None): the triangles of
    the whole mesh that the line through each point along ``axis`` crosses above, below and exactly at the point.  order = the
    permutation in which the points are worked on (or None); n_tests (int64 [1]) accumulates the number of line-triangle tests."""
    _tptr(points, 'mesh_crossings: points', torch.float64)
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError('mesh_crossings: points [Q, 3] expected, got %s' % (tuple(points.shape),))
    q = points.shape[0]
    assert order is None or order.numel() == q
    dev = points.device
    above = torch.empty(q, dtype=torch.int32, device=dev)
    below = torch.empty(q, dtype=torch.int32, device=dev) if want_below else None
    on = torch.empty(q, dtype=torch.int32, device=dev) if want_on else None
    with _Prof('mesh_crossings', q):
        _check(_lib.psn_mesh_crossings(ctypes.byref(index), points.data_ptr(),
                                       None if order is None else _tptr(order, 'order', torch.int64), q, int(axis),
                                       above.data_ptr(), None if below is None else below.data_ptr(), None if on is None else on.data_ptr(),
                                       None if n_tests is None else _tptr(n_tests, 'n_tests', torch.int64), _stream()), 'mesh_crossings')
    return above, below, on


# --------------------------------------------------------------------------- mesh clean-up (csrc/meshclean.hip)
def cc_label(faces, n_vertices, status):
    """psn_cc_label: faces int64 [F, 3] -> labels int32 [n_vertices], the smallest vertex index reachable from each vertex.  status
    (int32 [1] on the device) is set: CC_E_* bits; the caller reads it together with the table (meshclean._device_table)."""
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError('cc_label: faces [F, 3] expected, got %s' % (tuple(faces.shape),))
    n_v, n_f = int(n_vertices), faces.shape[0]
    assert status.numel() == 1
    parent = torch.empty(n_v, dtype=torch.int32, device=faces.device)
    labels = torch.empty(n_v, dtype=torch.int32, device=faces.device)
    with _Prof('cc_label', 24 * n_f + 12 * n_v):   # faces read once; parent written, read and the labels written
        _check(_lib.psn_cc_label(_tptr(faces, 'faces', torch.int64), n_f, n_v, parent.data_ptr(), labels.data_ptr(),
                                 _tptr(status, 'status', torch.int32), _stream()), 'cc_label')
    return labels


def cc_stats(vertices, faces, labels, status):
    """psn_cc_stats -> (counts int64 [2, V]: vertices and faces per component, area float64 [V]), indexed by the component's label."""
    vp, fp = _mesh_ptrs(vertices, faces)
    n_v, n_f = vertices.shape[0], faces.shape[0]
    assert labels.numel() == n_v and status.numel() == 1
    counts = torch.empty(2, n_v, dtype=torch.int64, device=vertices.device)
    area = torch.empty(n_v, dtype=torch.float64, device=vertices.device)
    with _Prof('cc_stats', 28 * n_v + 96 * n_f):   # labels read, three tables zeroed; per face its indices and three vertices
        _check(_lib.psn_cc_stats(vp, fp, n_f, n_v, _tptr(labels, 'labels', torch.int32), counts[0].data_ptr(), counts[1].data_ptr(),
                                 area.data_ptr(), _tptr(status, 'status', torch.int32), _stream()), 'cc_stats')
    return counts, area


def cc_flag(faces, labels, keep_label):
    """psn_cc_flag: keep_label uint8 [V] (per label) -> (face_keep uint8 [F], vertex_keep uint8 [V])."""
    n_v, n_f = labels.numel(), faces.shape[0]
    assert keep_label.numel() == n_v
    face_keep = torch.empty(n_f, dtype=torch.uint8, device=faces.device)
    vertex_keep = torch.empty(n_v, dtype=torch.uint8, device=faces.device)
    with _Prof('cc_flag', 29 * n_f + n_v):
        _check(_lib.psn_cc_flag(_tptr(faces, 'faces', torch.int64), n_f, n_v, _tptr(labels, 'labels', torch.int32),
                                _tptr(keep_label, 'keep_label', torch.uint8), face_keep.data_ptr(), vertex_keep.data_ptr(), _stream()), 'cc_flag')
    return face_keep, vertex_keep


def cc_compact(vertices, faces, normals, face_keep, vertex_keep, face_pos, vertex_pos, n_out_faces, n_out_vertices):
    """psn_cc_compact -> (vertices float64 [n_out_vertices, 3], faces int64 [n_out_faces, 3], normals or None): what the flags keep, in
    the original order, faces re-indexed.  face_pos / vertex_pos: the int64 exclusive scans of the flags; normals float32 or float64."""
    vp, fp = _mesh_ptrs(vertices, faces)
    n_v, n_f = vertices.shape[0], faces.shape[0]
    assert face_keep.numel() == face_pos.numel() == n_f and vertex_keep.numel() == vertex_pos.numel() == n_v
    dev = vertices.device
    out_v = torch.empty(int(n_out_vertices), 3, dtype=torch.float64, device=dev)
    out_f = torch.empty(int(n_out_faces), 3, dtype=torch.int64, device=dev)
    out_n, nb = None, 0
    if normals is not None:
        if tuple(normals.shape) != (n_v, 3):
            raise RuntimeError('cc_compact: normals [%d, 3] expected, got %s' % (n_v, tuple(normals.shape)))
        nb = normals.element_size()
        out_n = torch.empty(int(n_out_vertices), 3, dtype=normals.dtype, device=dev)
    with _Prof('cc_compact', 9 * n_v + 9 * n_f + (48 + 2 * 3 * nb) * int(n_out_vertices) + 72 * int(n_out_faces)):
        _check(_lib.psn_cc_compact(vp, None if normals is None else _tptr(normals, 'normals', (torch.float32, torch.float64)), nb, fp, n_f, n_v,
                                   _tptr(face_keep, 'face_keep', torch.uint8), _tptr(vertex_keep, 'vertex_keep', torch.uint8),
                                   _tptr(face_pos, 'face_pos', torch.int64), _tptr(vertex_pos, 'vertex_pos', torch.int64), int(n_out_faces),
                                   int(n_out_vertices), out_v.data_ptr(), None if out_n is None else out_n.data_ptr(), out_f.data_ptr(),
                                   _stream()), 'cc_compact')
    return out_v, out_f, out_n


# --------------------------------------------------------------------------- mesh simplification (csrc/meshsimplify.hip)
def _vc_grid(grid):
    """(origin, h, dims) of meshsimplify.make_grid -> the seven scalars of the C ABI."""
    origin, h, dims = grid
    return float(origin[0]), float(origin[1]), float(origin[2]), float(h), int(dims[0]), int(dims[1]), int(dims[2])


def vc_cell_keys(vertices, grid):
    """psn_vc_cell_keys: vertices float64 [V, 3] -> keys int64 [V], the key of each vertex's grid cell."""
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError('vc_cell_keys: vertices [V, 3] expected, got %s' % (tuple(vertices.shape),))
    n_v = vertices.shape[0]
    keys = torch.empty(n_v, dtype=torch.int64, device=vertices.device)
    with _Prof('vc_cell_keys', 32 * n_v):
        _check(_lib.psn_vc_cell_keys(_tptr(vertices, 'vertices', torch.float64), n_v, *_vc_grid(grid), keys.data_ptr(), _stream()), 'vc_cell_keys')
    return keys


def vc_face_keys(faces, cluster, status, want_corners=True):
    """psn_vc_face_keys: faces int64 [F, 3], cluster int64 [V] -> (corner_keys int64 [3 F] or None, face_keys int64 [F], g int64 [F, 3]).
    status (int32 [1] on the device, zeroed by the caller) collects VC_E_* bits; the caller reads it with its counts."""
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError('vc_face_keys: faces [F, 3] expected, got %s' % (tuple(faces.shape),))
    n_f, n_v = faces.shape[0], cluster.numel()
    assert status.numel() == 1
    dev = faces.device
    corner_keys = torch.empty(3 * n_f, dtype=torch.int64, device=dev) if want_corners else None
    face_keys = torch.empty(n_f, dtype=torch.int64, device=dev)
    g = torch.empty(n_f, 3, dtype=torch.int64, device=dev)
    with _Prof('vc_face_keys', (24 + 24 + 8 + 24 + (24 if want_corners else 0)) * n_f):
        _check(_lib.psn_vc_face_keys(_tptr(faces, 'faces', torch.int64), n_f, n_v, _tptr(cluster, 'cluster', torch.int64),
                                     None if corner_keys is None else corner_keys.data_ptr(), face_keys.data_ptr(), g.data_ptr(),
                                     _tptr(status, 'status', torch.int32), _stream()), 'vc_face_keys')
    return corner_keys, face_keys, g


def vc_solve(vertices, faces, vertex_order, vertex_start, cell_key_sorted, corner_sorted, corner_start, n_clusters, grid, regularisation):
    """psn_vc_solve -> (positions float64 [C, 3], clamped uint8 [C]): per cluster the centroid over its vertex run, the quadric over its
    corner run, the solve and the clamp, every sum in the definition's order."""
    vp, fp = _mesh_ptrs(vertices, faces)
    n_v, n_f, n_c = vertices.shape[0], faces.shape[0], int(n_clusters)
    assert vertex_order.numel() == cell_key_sorted.numel() == n_v and corner_sorted.numel() == 3 * n_f
    assert vertex_start.numel() == corner_start.numel() == n_c + 1
    positions = torch.empty(n_c, 3, dtype=torch.float64, device=vertices.device)
    clamped = torch.empty(n_c, dtype=torch.uint8, device=vertices.device)
    with _Prof('vc_solve', 32 * n_v + 3 * n_f * (8 + 24 + 72) + 25 * n_c):
        _check(_lib.psn_vc_solve(vp, fp, n_f, n_v, _tptr(vertex_order, 'vertex_order', torch.int64), _tptr(vertex_start, 'vertex_start', torch.int64),
                                 _tptr(cell_key_sorted, 'cell_key_sorted', torch.int64), _tptr(corner_sorted, 'corner_sorted', torch.int64),
                                 _tptr(corner_start, 'corner_start', torch.int64), n_c, *_vc_grid(grid), float(regularisation),
                                 positions.data_ptr(), clamped.data_ptr(), _stream()), 'vc_solve')
    return positions, clamped


def vc_face_flags(vertices, faces, g, positions, face_keep):
    """psn_vc_face_flags -> (vertex_keep uint8 [C]: the clusters a kept face names, flipped uint8 [F]: kept faces whose normal turned)."""
    vp, fp = _mesh_ptrs(vertices, faces)
    n_v, n_f, n_c = vertices.shape[0], faces.shape[0], positions.shape[0]
    assert g.numel() == 3 * n_f and face_keep.numel() == n_f
    vertex_keep = torch.empty(n_c, dtype=torch.uint8, device=vertices.device)
    flipped = torch.empty(n_f, dtype=torch.uint8, device=vertices.device)
    with _Prof('vc_face_flags', n_c + n_f * (2 + 48 + 144)):
        _check(_lib.psn_vc_face_flags(vp, fp, n_f, n_v, _tptr(g, 'g', torch.int64), _tptr(positions, 'positions', torch.float64), n_c,
                                      _tptr(face_keep, 'face_keep', torch.uint8), vertex_keep.data_ptr(), flipped.data_ptr(), _stream()),
               'vc_face_flags')
    return vertex_keep, flipped


# --------------------------------------------------------------------------- mesh connectivity and smoothing (csrc/meshtopo.hip)
def _faces_ptr(faces, what, stand_in):
    """Device pointer of faces int64 [F, 3]; F may be 0 (``stand_in``: see _eptr)."""
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError('%s: faces [F, 3] expected, got %s' % (what, tuple(faces.shape)))
    _tptr(faces, 'faces', torch.int64)
    return _eptr(faces, stand_in)


def topo_edge_keys(faces, n_vertices, status, out=None):
    """psn_topo_edge_keys: faces int64 [F, 3] -> keys int64 [3 F], min(a, b) V + max(a, b) per half-edge h = 3 f + k, INT64_MAX for a
    degenerate or skipped face.  status (int32 [1] on the device, zeroed by the caller) collects TOPO_E_* bits."""
    fp = _faces_ptr(faces, 'topo_edge_keys', status)
    n_f = faces.shape[0]
    assert status.numel() == 1
    keys = _out(out, (3 * n_f,), faces, 'topo_edge_keys', torch.int64)
    with _Prof('topo_edge_keys', 48 * n_f):
        _check(_lib.psn_topo_edge_keys(fp, n_f, int(n_vertices), _eptr(keys, status), _tptr(status, 'status', torch.int32), _stream()),
               'topo_edge_keys')
    return keys


def topo_edges(sorted_keys, order, rank_incl, faces, n_vertices, n_edges, out=None):
    """psn_topo_edges: the stable sort of the half-edge keys, its permutation and the inclusive head-flag scan -> (edges int64 [E, 2],
    count int32 [E], forward int32 [E], halfedge_edge int64 [3 F], vertex_used uint8 [V], vertex_open uint8 [V], counters int64 [4]:
    boundary, non-manifold, inconsistent edges and degenerate faces).  ``out``: a tuple of the seven, or None."""
    n_f, n_v, n_e = faces.shape[0], int(n_vertices), int(n_edges)
    assert sorted_keys.numel() == order.numel() == rank_incl.numel() == 3 * n_f
    for t, name in ((sorted_keys, 'sorted_keys'), (order, 'order'), (rank_incl, 'rank_incl')):
        _tptr(t, name, torch.int64)
    out = (None,) * 7 if out is None else out
    edges = _out(out[0], (n_e, 2), faces, 'topo_edges: edges', torch.int64)
    count = _out(out[1], (n_e,), faces, 'topo_edges: count', torch.int32)
    forward = _out(out[2], (n_e,), faces, 'topo_edges: forward', torch.int32)
    halfedge_edge = _out(out[3], (3 * n_f,), faces, 'topo_edges: halfedge_edge', torch.int64)
    used = _out(out[4], (n_v,), faces, 'topo_edges: vertex_used', torch.uint8)
    is_open = _out(out[5], (n_v,), faces, 'topo_edges: vertex_open', torch.uint8)
    counters = _out(out[6], (4,), faces, 'topo_edges: counters', torch.int64)
    fp = _faces_ptr(faces, 'topo_edges', counters)
    with _Prof('topo_edges', 3 * n_f * (8 + 8 + 8 + 16 + 8) + n_e * 24 + 2 * n_v):
        _check(_lib.psn_topo_edges(_eptr(sorted_keys, counters), _eptr(order, counters), _eptr(rank_incl, counters), fp, n_f, n_v, n_e,
                                   _eptr(edges, counters), _eptr(count, counters), _eptr(forward, counters), _eptr(halfedge_edge, counters),
                                   _eptr(used, counters), _eptr(is_open, counters), counters.data_ptr(), _stream()), 'topo_edges')
    return edges, count, forward, halfedge_edge, used, is_open, counters


def topo_ring_keys(edges, n_vertices):
    """psn_topo_ring_keys: edges int64 [E, 2] -> keys int64 [2 E], the directed pairs lo V + hi and hi V + lo."""
    if edges.dim() != 2 or edges.shape[1] != 2:
        raise RuntimeError('topo_ring_keys: edges [E, 2] expected, got %s' % (tuple(edges.shape),))
    _tptr(edges, 'edges', torch.int64)
    n_e = edges.shape[0]
    keys = torch.empty(2 * n_e, dtype=torch.int64, device=edges.device)
    if n_e:
        with _Prof('topo_ring_keys', 32 * n_e):
            _check(_lib.psn_topo_ring_keys(edges.data_ptr(), n_e, int(n_vertices), keys.data_ptr(), _stream()), 'topo_ring_keys')
    return keys


def topo_corner_keys(faces, n_vertices, status):
    """psn_topo_corner_keys: faces int64 [F, 3] -> keys int64 [3 F], corner-major: keys[k F + f] = f[k] (V for a skipped face)."""
    fp = _faces_ptr(faces, 'topo_corner_keys', status)
    n_f = faces.shape[0]
    assert status.numel() == 1
    keys = torch.empty(3 * n_f, dtype=torch.int64, device=faces.device)
    with _Prof('topo_corner_keys', 48 * n_f):
        _check(_lib.psn_topo_corner_keys(fp, n_f, int(n_vertices), _eptr(keys, status), _tptr(status, 'status', torch.int32), _stream()),
               'topo_corner_keys')
    return keys


def topo_runs(sorted_keys, div, n_vertices, want_rem=False, out=None):
    """psn_topo_runs: ascending keys int64 [n] -> (start int64 [V + 1]: the first position whose key // div is >= x, rem int64 [n] =
    key % div or None).  ``out``: a tuple (start, rem or None), or None."""
    n, n_v = sorted_keys.numel(), int(n_vertices)
    _tptr(sorted_keys, 'sorted_keys', torch.int64)
    out = (None, None) if out is None else out
    start = _out(out[0], (n_v + 1,), sorted_keys, 'topo_runs: start', torch.int64)
    rem = _out(out[1], (n,), sorted_keys, 'topo_runs: rem', torch.int64) if want_rem else None
    with _Prof('topo_runs', (8 + (8 if want_rem else 0)) * n + 8 * (n_v + 1)):
        _check(_lib.psn_topo_runs(_eptr(sorted_keys, start), n, int(div), n_v, start.data_ptr(), None if rem is None else _eptr(rem, start),
                                  _stream()), 'topo_runs')
    return start, rem


TOPO_WEIGHTS = {'area': TOPO_WEIGHT_AREA, 'uniform': TOPO_WEIGHT_UNIFORM}  # noqa: F821


def topo_vertex_normals(vertices, faces, corner_start, corner, weight='area', out=None):
    """psn_topo_vertex_normals -> normals float64 [V, 3]: per vertex the normalised sum over its corner run (in the run's order, from
    +0.0) of its faces' cross products ('area') or unit normals ('uniform')."""
    if weight not in TOPO_WEIGHTS:
        raise ValueError("vertex normals: weight=%r ('area' or 'uniform')" % (weight,))
    _mesh_ptrs(vertices, faces)
    n_v, n_f = vertices.shape[0], faces.shape[0]
    assert corner_start.numel() == n_v + 1 and corner.numel() == 3 * n_f
    normals = _out(out, (n_v, 3), vertices, 'topo_vertex_normals', torch.float64)
    _tptr(corner, 'corner', torch.int64)
    if n_v:
        with _Prof('topo_vertex_normals', n_v * (16 + 24) + 3 * n_f * (8 + 24 + 72)):
            _check(_lib.psn_topo_vertex_normals(vertices.data_ptr(), _eptr(faces, vertices), n_f, n_v, _tptr(corner_start, 'corner_start', torch.int64),
                                                _eptr(corner, vertices), TOPO_WEIGHTS[weight], normals.data_ptr(), _stream()),
                   'topo_vertex_normals')
    return normals


def topo_smooth_step(x, ring_start, ring, pinned, s, out=None):
    """psn_topo_smooth_step: x float64 [V, 3] -> out [V, 3] = x + s (ring mean - x) per vertex with a non-empty ring that is not pinned
    (pinned uint8 [V] or None); the other vertices keep their bits."""
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError('topo_smooth_step: x [V, 3] expected, got %s' % (tuple(x.shape),))
    _tptr(x, 'x', torch.float64)
    n_v, n_r = x.shape[0], ring.numel()
    assert ring_start.numel() == n_v + 1 and (pinned is None or pinned.numel() == n_v)
    out = _out(out, (n_v, 3), x, 'topo_smooth_step', torch.float64)
    if n_v:
        _tptr(ring, 'ring', torch.int64)
        with _Prof('topo_smooth_step', n_v * (16 + 1 + 48) + n_r * 32):
            _check(_lib.psn_topo_smooth_step(x.data_ptr(), n_v, _tptr(ring_start, 'ring_start', torch.int64), _eptr(ring, x), n_r,
                                             None if pinned is None else _tptr(pinned, 'pinned', torch.uint8), float(s), out.data_ptr(),
                                             _stream()), 'topo_smooth_step')
    return out


def topo_measures(vertices, faces, out=None):
    """psn_topo_measures -> float64 [2] on the device: area and signed volume (fixed summation order; no atomics)."""
    _mesh_ptrs(vertices, faces)
    n_v, n_f = vertices.shape[0], faces.shape[0]
    out = _out(out, (2,), vertices, 'topo_measures', torch.float64)
    partial = torch.empty(2 * TOPO_MEASURE_BLOCKS, dtype=torch.float64, device=vertices.device)  # noqa: F821
    with _Prof('topo_measures', 96 * n_f):
        _check(_lib.psn_topo_measures(_eptr(vertices, partial), _eptr(faces, partial), n_f, n_v, partial.data_ptr(), out.data_ptr(), _stream()),
               'topo_measures')
    return out


# --------------------------------------------------------------------------- image evaluation (csrc/imgmetrics.hip)
IMG_TYPES = {torch.float32: IMG_F32, torch.uint8: IMG_U8}  # noqa: F821


def _img_pair(what, pred, gt, mask):
    """The checks every image entry shares -> (image_type, mask pointer or None, mask batch, B, H, W)."""
    for name, t in (('pred', pred), ('gt', gt)):
        _tptr(t, '%s: %s' % (what, name), tuple(IMG_TYPES))
        if t.dim() != 4 or t.shape[3] != 3:
            raise RuntimeError('%s: %s [B, H, W, 3] expected, got %s' % (what, name, tuple(t.shape)))
    if pred.dtype != gt.dtype:
        raise RuntimeError('%s: pred is %s and gt is %s (one dtype for the pair)' % (what, pred.dtype, gt.dtype))
    if pred.shape != gt.shape:
        raise RuntimeError('%s: shape mismatch, pred %s and gt %s' % (what, tuple(pred.shape), tuple(gt.shape)))
    B, H, W = (int(x) for x in pred.shape[:3])
    if B < 1 or H < IMG_MIN_EXTENT or W < IMG_MIN_EXTENT:
        raise RuntimeError('%s: %d images of %d x %d pixels (at least one, and at least %d pixels per extent: the 11-tap window must fit)'
                           % (what, B, H, W, IMG_MIN_EXTENT))
    mp, mb = _mask_ptr(what, mask, B, (H, W), pred.device)
    return IMG_TYPES[pred.dtype], mp, mb, B, H, W


def _mask_ptr(what, mask, B, tail, device):
    """mask: None, or a uint8 / bool device tensor [B or 1, *tail] -> (pointer or None, mask batch)."""
    if mask is None:
        return None, 1
    ptr = _tptr(mask, '%s: mask' % what, (torch.uint8, torch.bool))
    if mask.dim() != 1 + len(tail) or tuple(mask.shape[1:]) != tuple(tail):
        raise RuntimeError('%s: mask [B or 1, %s] expected, got %s' % (what, ', '.join(str(x) for x in tail), tuple(mask.shape)))
    if mask.shape[0] not in (1, B):
        raise RuntimeError('%s: mask batch %d is neither 1 nor B = %d' % (what, mask.shape[0], B))
    if mask.device != device:
        raise RuntimeError('%s: mask must be on the images\' device' % what)
    return ptr, int(mask.shape[0])


def _img_partial(which, B, H, W, device):
    n = int(_lib.psn_img_workspace(which, B, H, W))
    if n < 0:
        raise RuntimeError('psn_img_workspace(%d, %d, %d, %d) refused' % (which, B, H, W))
    return torch.empty(n, dtype=torch.float64, device=device)


def img_scale_sums(pred, gt, mask):
    """psn_img_scale_sums: pred / gt [B, H, W, 3] (float32 or uint8), mask [B or 1, H, W] (uint8 / bool) or None ->
    (sums float64 [B, 7] = masked sum of pred * gt per channel, of pred * pred per channel, masked pixels; partial rows)."""
    ty, mp, mb, B, H, W = _img_pair('img_scale_sums', pred, gt, mask)
    partial = _img_partial(IMG_WS_SCALE_SUMS, B, H, W, pred.device)
    sums = torch.empty(B, 7, dtype=torch.float64, device=pred.device)
    with _Prof('img_scale_sums', B * H * W * (2 * 3 * pred.element_size() + 1)):
        _check(_lib.psn_img_scale_sums(pred.data_ptr(), gt.data_ptr(), ty, mp, mb, B, H, W, partial.data_ptr(), sums.data_ptr(), _stream()),
               'img_scale_sums')
    return sums, partial


def img_metrics(pred, gt, mask, scale=None, full=False):
    """psn_img_metrics, the fused pass: pred / gt [B, H, W, 3] (float32 or uint8), mask [B or 1, H, W] or None, scale float64 [B] or
    None -> dict(ssim [B], psnr [B], sums [B, 7], partial, map [B, H, W, 3] or None), all float64 device tensors."""
    ty, mp, mb, B, H, W = _img_pair('img_metrics', pred, gt, mask)
    dev = pred.device
    sp = _tptr(scale, 'img_metrics: scale', torch.float64, allow_none=True)
    if scale is not None and tuple(scale.shape) != (B,):
        raise RuntimeError('img_metrics: scale [%d] expected, got %s' % (B, tuple(scale.shape)))
    partial = _img_partial(IMG_WS_METRICS, B, H, W, dev)
    sums = torch.empty(B, 7, dtype=torch.float64, device=dev)
    ssim = torch.empty(B, dtype=torch.float64, device=dev)
    psnr = torch.empty(B, dtype=torch.float64, device=dev)
    smap = torch.empty(B, H, W, 3, dtype=torch.float64, device=dev) if full else None
    with _Prof('img_metrics', B * H * W * (2 * 3 * pred.element_size() + 1)):   # the compulsory bytes: two images and one mask
        _check(_lib.psn_img_metrics(pred.data_ptr(), gt.data_ptr(), ty, mp, mb, sp, B, H, W,
                                    partial.data_ptr(), sums.data_ptr(), ssim.data_ptr(), psnr.data_ptr(),
                                    None if smap is None else smap.data_ptr(), _stream()), 'img_metrics')
    return {'ssim': ssim, 'psnr': psnr, 'sums': sums, 'partial': partial, 'map': smap}


def normal_mae(pred, gt, mask, normalize=True, full=False):
    """psn_normal_mae: pred / gt float32 [B, N, 3] normal maps, mask [B or 1, N] (uint8 / bool) or None -> (sums float64 [B, 2] =
    masked sum of the angular errors in degrees, masked pixels; partial rows; per-pixel errors [B, N] or None)."""
    for name, t in (('pred', pred), ('gt', gt)):
        _tptr(t, 'normal_mae: %s' % name)
        if t.dim() != 3 or t.shape[2] != 3:
            raise RuntimeError('normal_mae: %s: [B, N, 3] expected, got %s' % (name, tuple(t.shape)))
    if pred.shape != gt.shape:
        raise RuntimeError('normal_mae: shape mismatch, pred %s and gt %s' % (tuple(pred.shape), tuple(gt.shape)))
    B, N = int(pred.shape[0]), int(pred.shape[1])
    if B < 1 or N < 1:
        raise RuntimeError('normal_mae: empty input %s' % (tuple(pred.shape),))
    mp, mb = _mask_ptr('normal_mae', mask, B, (N,), pred.device)
    partial = _img_partial(IMG_WS_NORMAL_MAE, B, 1, N, pred.device)
    sums = torch.empty(B, 2, dtype=torch.float64, device=pred.device)
    err = torch.empty(B, N, dtype=torch.float64, device=pred.device) if full else None
    with _Prof('normal_mae', B * N * 25):
        _check(_lib.psn_normal_mae(pred.data_ptr(), gt.data_ptr(), mp, mb, int(bool(normalize)), B, N, partial.data_ptr(), sums.data_ptr(),
                                   None if err is None else err.data_ptr(), _stream()), 'normal_mae')
    return sums, partial, err


# --------------------------------------------------------------------------- photometric stereo (csrc/photostereo.hip)
PS_PATHS = {'auto': PS_PATH_AUTO, 'tile': PS_PATH_TILE, 'reform': PS_PATH_REFORM}  # noqa: F821


def _ps_images(what, images, mask):
    """The checks every photometric-stereo entry shares -> (image_type, mask pointer or None, L, n_pixels)."""
    _tptr(images, '%s: images' % what, tuple(IMG_TYPES))
    if images.dim() != 3 or images.shape[2] != 3:
        raise RuntimeError('%s: images [L, n_pixels, 3] expected, got %s' % (what, tuple(images.shape)))
    L, N = int(images.shape[0]), int(images.shape[1])
    if not PS_MIN_LIGHTS <= L <= PS_MAX_LIGHTS or N < 1:  # noqa: F821
        raise RuntimeError('%s: %d lights (%d .. %d) of %d pixels (at least one)' % (what, L, PS_MIN_LIGHTS, PS_MAX_LIGHTS, N))  # noqa: F821
    mp = _tptr(mask, '%s: mask' % what, (torch.uint8, torch.bool), allow_none=True)
    if mask is not None and (tuple(mask.shape) != (N,) or mask.device != images.device):
        raise RuntimeError('%s: mask [%d] on the images\' device expected, got %s' % (what, N, tuple(mask.shape)))
    return IMG_TYPES[images.dtype], mp, L, N


def _ps_table(what, name, t, L, device, allow_none=False):
    """A float64 [L, 3] device table (light directions, intensities) -> pointer or None."""
    ptr = _tptr(t, '%s: %s' % (what, name), torch.float64, allow_none=allow_none)
    if t is not None and (tuple(t.shape) != (L, 3) or t.device != device):
        raise RuntimeError('%s: %s [%d, 3] on the images\' device expected, got %s' % (what, name, L, tuple(t.shape)))
    return ptr


def ps_normals(images, mask, light_dir, light_int=None, low=0.1, high=0.25, dark=0.0, min_lights=3, cond=1e-4, path='auto', out=None):
    """psn_ps_normals: images [L, N, 3] (uint8 or float32), mask [N] (uint8 / bool) or None, light_dir float64 [L, 3], light_int float64
    [L, 3] or None -> (normal float64 [N, 3], albedo float64 [N, 3], valid uint8 [N], kept int32 [N]); ``out``: the four, preallocated."""
    ty, mp, L, N = _ps_images('ps_normals', images, mask)
    dev = images.device
    if path not in PS_PATHS:
        raise RuntimeError('ps_normals: path %r (auto, tile, reform)' % (path,))
    o = out if out is not None else (None, None, None, None)
    normal = _out(o[0], (N, 3), images, 'ps_normals: normal', torch.float64)
    albedo = _out(o[1], (N, 3), images, 'ps_normals: albedo', torch.float64)
    valid = _out(o[2], (N,), images, 'ps_normals: valid', torch.uint8)
    kept = _out(o[3], (N,), images, 'ps_normals: kept', torch.int32)
    with _Prof('ps_normals', L * N * 3 * images.element_size()):
        _check(_lib.psn_ps_normals(images.data_ptr(), ty, mp, _ps_table('ps_normals', 'light_dir', light_dir, L, dev),
                                   _ps_table('ps_normals', 'light_int', light_int, L, dev, allow_none=True), L, N, float(low), float(high),
                                   float(dark), int(min_lights), float(cond), PS_PATHS[path], normal.data_ptr(), albedo.data_ptr(),
                                   valid.data_ptr(), kept.data_ptr(), _stream()), 'ps_normals')
    return normal, albedo, valid, kept


def ps_light_intensity(images, normal, albedo, valid, light_dir, dark=0.0, bright=1.0, out=None):
    """psn_ps_light_intensity: images [L, N, 3], normal / albedo float64 [N, 3], valid [N] (uint8 / bool), light_dir float64 [L, 3] ->
    (intensity float64 [L, 3], sums float64 [L, 6], partial rows); ``out``: (intensity, sums), preallocated."""
    ty, vp, L, N = _ps_images('ps_light_intensity', images, valid)
    dev = images.device
    if valid is None:
        raise RuntimeError('ps_light_intensity: valid: tensor required')
    for name, t in (('normal', normal), ('albedo', albedo)):
        _tptr(t, 'ps_light_intensity: %s' % name, torch.float64)
        if tuple(t.shape) != (N, 3) or t.device != dev:
            raise RuntimeError('ps_light_intensity: %s [%d, 3] on the images\' device expected, got %s' % (name, N, tuple(t.shape)))
    n = int(_lib.psn_ps_workspace(L, N))
    if n < 0:
        raise RuntimeError('psn_ps_workspace(%d, %d) refused' % (L, N))
    partial = torch.empty(n, dtype=torch.float64, device=dev)
    o = out if out is not None else (None, None)
    intensity = _out(o[0], (L, 3), images, 'ps_light_intensity: intensity', torch.float64)
    sums = _out(o[1], (L, 6), images, 'ps_light_intensity: sums', torch.float64)
    with _Prof('ps_light_intensity', L * N * (3 * images.element_size() + 49)):
        _check(_lib.psn_ps_light_intensity(images.data_ptr(), ty, normal.data_ptr(), albedo.data_ptr(), vp,
                                           _ps_table('ps_light_intensity', 'light_dir', light_dir, L, dev), L, N, float(dark), float(bright),
                                           partial.data_ptr(), sums.data_ptr(), intensity.data_ptr(), _stream()), 'ps_light_intensity')
    return intensity, sums, partial


def ps_light_average(images, mask, relat_int=None, normalised=None, out=None):
    """psn_ps_light_average: images [L, N, 3], mask [N] or None, relat_int float64 [L, 3] or None -> (mean float64 [N, 3], mean_u8 [N, 3],
    the normalised images uint8 [L, N, 3] or None); ``normalised``: whether to write those (default: when relat_int is given); ``out``:
    (mean, mean_u8, normalised images or None), preallocated."""
    ty, mp, L, N = _ps_images('ps_light_average', images, mask)
    dev = images.device
    o = out if out is not None else (None, None, None)
    mean = _out(o[0], (N, 3), images, 'ps_light_average: mean', torch.float64)
    mean_u8 = _out(o[1], (N, 3), images, 'ps_light_average: mean_u8', torch.uint8)
    want = (relat_int is not None) if normalised is None else bool(normalised)
    norm = _out(o[2], (L, N, 3), images, 'ps_light_average: normalised images', torch.uint8) if want else None
    with _Prof('ps_light_average', L * N * 3 * images.element_size() * (2 if want else 1)):
        _check(_lib.psn_ps_light_average(images.data_ptr(), ty, mp, _ps_table('ps_light_average', 'relat_int', relat_int, L, dev, allow_none=True),
                                         L, N, mean.data_ptr(), mean_u8.data_ptr(), None if norm is None else norm.data_ptr(), _stream()),
               'ps_light_average')
    return mean, mean_u8, norm


# --------------------------------------------------------------------------- texture atlas of a mesh (csrc/meshbake.hip)
def _atlas_texture(what, tex, T):
    """A [T, T, C] float32 or uint8 device texture -> (pointer, C, texture type)."""
    ptr = _tptr(tex, '%s: texture' % what, tuple(IMG_TYPES))
    if tex.dim() != 3 or tex.shape[0] != T or tex.shape[1] != T or not 1 <= tex.shape[2] <= ATLAS_MAX_CHANNELS:  # noqa: F821
        raise RuntimeError('%s: texture [%d, %d, 1 .. %d] expected, got %s' % (what, T, T, ATLAS_MAX_CHANNELS, tuple(tex.shape)))  # noqa: F821
    return ptr, int(tex.shape[2]), IMG_TYPES[tex.dtype]


def atlas_points(vertices, faces, vertex_normals, T, cell, f0=0, f1=None, out=None):
    """psn_atlas_points: vertices float64 [V, 3], faces int64 [F, 3], vertex_normals float64 [V, 3] or None; the rows of the faces
    f0 <= f < f1 -> (points float64 [R, 3], points_f32 float32 [R, 3], normals float64 [R, 3]), R = (f1 - f0) K; ``out``: the three,
    preallocated."""
    vp, fp = _mesh_ptrs(vertices, faces)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    f1 = F if f1 is None else int(f1)
    f0 = int(f0)
    np_ = _tptr(vertex_normals, 'atlas_points: vertex_normals', torch.float64, allow_none=True)
    if vertex_normals is not None and (tuple(vertex_normals.shape) != (V, 3) or vertex_normals.device != vertices.device):
        raise RuntimeError('atlas_points: vertex_normals [%d, 3] on the mesh\'s device expected, got %s' % (V, tuple(vertex_normals.shape)))
    if not (cell >= ATLAS_MIN_CELL and 0 <= f0 <= f1 <= F):  # noqa: F821
        raise RuntimeError('atlas_points: cell %d (at least %d), face range [%d, %d) of %d faces' % (cell, ATLAS_MIN_CELL, f0, f1, F))  # noqa: F821
    R = (f1 - f0) * ((cell - 1) * cell // 2)
    o = out if out is not None else (None, None, None)
    points = _out(o[0], (R, 3), vertices, 'atlas_points: points', torch.float64)
    points_f32 = _out(o[1], (R, 3), vertices, 'atlas_points: points_f32', torch.float32)
    normals = _out(o[2], (R, 3), vertices, 'atlas_points: normals', torch.float64)
    with _Prof('atlas_points', R):
        _check(_lib.psn_atlas_points(vp, V, fp, F, np_, int(T), int(cell), f0, f1, _eptr(points, vertices), _eptr(points_f32, vertices),
                                     _eptr(normals, vertices), _stream()), 'atlas_points')
    return points, points_f32, normals


def atlas_scatter(rows, texture, cell, n_faces, f0=0, f1=None):
    """psn_atlas_scatter: rows float32 [(f1 - f0) K, C] -> the texels of the faces f0 <= f < f1 of ``texture`` [T, T, C] (float32, or
    uint8 by the to_img rule), in place; no other texel is written."""
    T = int(texture.shape[0])
    tp, C, ty = _atlas_texture('atlas_scatter', texture, T)
    f1 = int(n_faces) if f1 is None else int(f1)
    f0 = int(f0)
    if not (cell >= ATLAS_MIN_CELL and 0 <= f0 <= f1 <= n_faces):  # noqa: F821
        raise RuntimeError('atlas_scatter: cell %d (at least %d), face range [%d, %d) of %d faces' % (cell, ATLAS_MIN_CELL, f0, f1, n_faces))  # noqa: F821
    R = (f1 - f0) * ((cell - 1) * cell // 2)
    _tptr(rows, 'atlas_scatter: rows')
    if tuple(rows.shape) != (R, C) or rows.device != texture.device:
        raise RuntimeError('atlas_scatter: rows [%d, %d] on the texture\'s device expected, got %s' % (R, C, tuple(rows.shape)))
    with _Prof('atlas_scatter', R * C * 4 + R * C * texture.element_size()):
        _check(_lib.psn_atlas_scatter(_eptr(rows, texture), C, T, int(cell), int(n_faces), f0, f1, tp, ty, _stream()), 'atlas_scatter')
    return texture


def atlas_fill(texture, cell, n_faces, fill=0.0):
    """psn_atlas_fill: the texels of ``texture`` [T, T, C] that no face owns := fill, in place (owned texels are left alone)."""
    T = int(texture.shape[0])
    tp, C, ty = _atlas_texture('atlas_fill', texture, T)
    with _Prof('atlas_fill', T * T * C * texture.element_size()):
        _check(_lib.psn_atlas_fill(float(fill), C, T, int(cell), int(n_faces), tp, ty, _stream()), 'atlas_fill')
    return texture


def atlas_sample(face, bary, texture, cell, n_faces, out=None):
    """psn_atlas_sample: face int64 [Q] (-1: a miss), bary float64 [Q, 3], texture float32 [T, T, C] -> float64 [Q, C], NaN rows for
    the misses."""
    T = int(texture.shape[0])
    tp, C, ty = _atlas_texture('atlas_sample', texture, T)
    if ty != IMG_F32:  # noqa: F821
        raise RuntimeError('atlas_sample: the texture must be float32, got %s' % texture.dtype)
    _tptr(face, 'atlas_sample: face', torch.int64)
    _tptr(bary, 'atlas_sample: bary', torch.float64)
    Q = int(face.shape[0])
    if face.dim() != 1 or tuple(bary.shape) != (Q, 3) or face.device != texture.device or bary.device != texture.device:
        raise RuntimeError('atlas_sample: face [Q] and bary [Q, 3] on the texture\'s device expected, got %s and %s' % (tuple(face.shape), tuple(bary.shape)))
    out = _out(out, (Q, C), texture, 'atlas_sample: out', torch.float64)
    with _Prof('atlas_sample', Q * C):
        _check(_lib.psn_atlas_sample(_eptr(face, texture), _eptr(bary, texture), Q, tp, C, T, int(cell), int(n_faces), _eptr(out, texture),
                                     _stream()), 'atlas_sample')
    return out


# --------------------------------------------------------------------------- silhouette carving (csrc/hull.hip)
def _hull_masks(what, masks):
    """A uint8 [V, H, W] device tensor of masks -> (pointer, V, H, W)."""
    ptr = _tptr(masks, '%s: masks' % what, torch.uint8)
    if masks.dim() != 3 or min(masks.shape) < 1:
        raise RuntimeError('%s: masks [V, H, W] (at least 1 x 1 x 1) expected, got %s' % (what, tuple(masks.shape)))
    return ptr, int(masks.shape[0]), int(masks.shape[1]), int(masks.shape[2])


def _hull_views(what, views, V, device):
    ptr = _tptr(views, '%s: views' % what, torch.float64)
    if tuple(views.shape) != (V, 16) or views.device != device:
        raise RuntimeError('%s: views [%d, 16] on the masks\' device expected, got %s' % (what, V, tuple(views.shape)))
    return ptr


def mask_dilate(masks, half_widths, border=0, invert=False, out=None):
    """psn_mask_dilate: masks uint8 [V, H, W] (non-0 = set), half_widths = a host table of 2 r + 1 integers -> uint8 0 / 1 [V, H, W];
    ``invert``: negate the input before and the output after (with border = 1: the erosion)."""
    mp, V, H, W = _hull_masks('mask_dilate', masks)
    table = [int(w) for w in half_widths]
    if len(table) % 2 != 1:
        raise RuntimeError('mask_dilate: a table of 2 r + 1 half-widths expected, got %d' % len(table))
    if any(not -2 ** 31 <= w < 2 ** 31 for w in table):
        raise RuntimeError('mask_dilate: a half-width outside the 32-bit range')
    n = int(_lib.psn_mask_dilate_workspace(V, H, W))
    if n < 0:
        raise RuntimeError('psn_mask_dilate_workspace(%d, %d, %d) refused' % (V, H, W))
    packed = torch.empty(n, dtype=torch.int64, device=masks.device)
    out = _out(out, (V, H, W), masks, 'mask_dilate: out', torch.uint8)
    with _Prof('mask_dilate', 2 * V * H * W):
        _check(_lib.psn_mask_dilate(mp, V, H, W, (ctypes.c_int32 * len(table))(*table), (len(table) - 1) // 2, int(border), int(bool(invert)),
                                    packed.data_ptr(), out.data_ptr(), _stream()), 'mask_dilate')
    return out


def hull_points(points, views, masks, out=None):
    """psn_hull_points: points float32 or float64 [Q, 3], views float64 [V, 16] (hull._views), masks uint8 [V, H, W] ->
    (keep uint8 [Q], carved_by int32 [Q]); ``out``: the two, preallocated."""
    mp, V, H, W = _hull_masks('hull_points', masks)
    _tptr(points, 'hull_points: points', (torch.float32, torch.float64))
    if points.dim() != 2 or points.shape[1] != 3 or points.device != masks.device:
        raise RuntimeError('hull_points: points [Q, 3] on the masks\' device expected, got %s' % (tuple(points.shape),))
    Q = int(points.shape[0])
    o = out if out is not None else (None, None)
    keep = _out(o[0], (Q,), masks, 'hull_points: keep', torch.uint8)
    carved_by = _out(o[1], (Q,), masks, 'hull_points: carved_by', torch.int32)
    with _Prof('hull_points', Q):
        _check(_lib.psn_hull_points(_eptr(points, masks), HULL_F32 if points.dtype == torch.float32 else HULL_F64, Q,  # noqa: F821
                                    _hull_views('hull_points', views, V, masks.device), V, mp, H, W, _eptr(keep, masks),
                                    _eptr(carved_by, masks), _stream()), 'hull_points')
    return keep, carved_by


def hull_grid(grid, axis, views, masks, value=-30.0):
    """psn_hull_grid, in place on grid float32 [n, n, n]: axis float64 [n], views float64 [V, 16], masks uint8 [V, H, W] -> the number
    of elements set to ``value``, int64 [1] on the device."""
    mp, V, H, W = _hull_masks('hull_grid', masks)
    gp = _tptr(grid, 'hull_grid: grid')
    n = int(grid.shape[0]) if grid.dim() == 3 else 0
    if tuple(grid.shape) != (n, n, n) or grid.device != masks.device:
        raise RuntimeError('hull_grid: a cubic grid [n, n, n] on the masks\' device expected, got %s' % (tuple(grid.shape),))
    ap = _tptr(axis, 'hull_grid: axis', torch.float64)
    if tuple(axis.shape) != (n,) or axis.device != masks.device:
        raise RuntimeError('hull_grid: axis [%d] on the masks\' device expected, got %s' % (n, tuple(axis.shape)))
    count = torch.zeros(1, dtype=torch.int64, device=masks.device)
    with _Prof('hull_grid', 4 * grid.numel()):
        _check(_lib.psn_hull_grid(gp, n, ap, _hull_views('hull_grid', views, V, masks.device), V, mp, H, W, float(value), count.data_ptr(),
                                  _stream()), 'hull_grid')
    return count


# --------------------------------------------------------------------------- mesh registration (csrc/meshalign.hip)
def _host_table(what, name, values, count):
    """A host table of ``count`` doubles (a rotation, a translation) as the C ABI takes it."""
    flat = [float(x) for row in values for x in (row if hasattr(row, '__len__') else (row,))]
    if len(flat) != count:
        raise RuntimeError('%s: %s: %d numbers expected, got %d' % (what, name, count, len(flat)))
    return (ctypes.c_double * count)(*flat)


def _align_rows(what, n, dev, **tensors):
    for name, t in tensors.items():
        _tptr(t, '%s: %s' % (what, name), torch.float64)
        if tuple(t.shape) != (n, 3) or t.device != dev:
            raise RuntimeError('%s: %s [%d, 3] on one device expected, got %s' % (what, name, n, tuple(t.shape)))


def align_transform(points, scale, rotation, translation, out=None):
    """psn_align_transform: points float64 [n, 3] -> scale (rotation x) + translation, float64 [n, 3], bit for bit
    meshalign.host_transform.  rotation [3, 3] and translation [3] are host values."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError('align_transform: points [n, 3] expected')
    n = int(points.shape[0])
    _align_rows('align_transform', n, points.device, points=points)
    out = _out(out, (n, 3), points, 'align_transform: out', torch.float64)
    R, t = _host_table('align_transform', 'rotation', rotation, 9), _host_table('align_transform', 'translation', translation, 3)
    if n:
        with _Prof('align_transform', 48 * n):
            _check(_lib.psn_align_transform(points.data_ptr(), n, float(scale), R, t, out.data_ptr(), _stream()), 'align_transform')
    return out


def align_dist(P, Y, out=None):
    """psn_align_dist: P, Y float64 [n, 3] -> |Y - P| float64 [n], bit for bit meshalign.host_dist."""
    if not isinstance(P, torch.Tensor) or P.dim() != 2:
        raise RuntimeError('align_dist: P [n, 3] expected')
    n = int(P.shape[0])
    _align_rows('align_dist', n, P.device, P=P, Y=Y)
    out = _out(out, (n,), P, 'align_dist: out', torch.float64)
    if n:
        with _Prof('align_dist', 56 * n):
            _check(_lib.psn_align_dist(P.data_ptr(), Y.data_ptr(), n, out.data_ptr(), _stream()), 'align_dist')
    return out


def align_sums(P, Y, tri, vertices, faces, max_dist, rotation=None, out=None):
    """psn_align_sums: rows P, Y float64 [n, 3], tri int64 [n], the mesh whose triangle normals are meant, max_dist (a host value),
    rotation = None or a host [3, 3] applied to the normals -> (sums float64 [ALIGN_SUMS], counts int64 [ALIGN_COUNTS], partial rows);
    ``out``: (sums, counts), preallocated."""
    if not isinstance(P, torch.Tensor) or P.dim() != 2:
        raise RuntimeError('align_sums: P [n, 3] expected')
    n, dev = int(P.shape[0]), P.device
    _align_rows('align_sums', n, dev, P=P, Y=Y)
    _tptr(tri, 'align_sums: tri', torch.int64)
    if tuple(tri.shape) != (n,) or tri.device != dev:
        raise RuntimeError('align_sums: tri [%d] on the rows\' device expected, got %s' % (n, tuple(tri.shape)))
    vp, fp = _mesh_ptrs(vertices, faces)
    if vertices.device != dev or faces.device != dev:
        raise RuntimeError('align_sums: the mesh must be on the rows\' device')
    words = int(_lib.psn_align_workspace(n))
    if words < 0:
        raise RuntimeError('psn_align_workspace(%d) refused' % n)
    partial = torch.empty(words, dtype=torch.float64, device=dev)
    o = out if out is not None else (None, None)
    sums = _out(o[0], (ALIGN_SUMS,), P, 'align_sums: sums', torch.float64)  # noqa: F821
    counts = _out(o[1], (ALIGN_COUNTS,), P, 'align_sums: counts', torch.int64)  # noqa: F821
    R = None if rotation is None else _host_table('align_sums', 'rotation', rotation, 9)
    with _Prof('align_sums', 64 * n):
        _check(_lib.psn_align_sums(_eptr(P, partial), _eptr(Y, partial), _eptr(tri, partial), n, vp, vertices.shape[0], fp, faces.shape[0], R,
                                   float(max_dist), partial.data_ptr(), sums.data_ptr(), counts.data_ptr(), _stream()), 'align_sums')
    return sums, counts, partial
