"""Host-side packing for the fused 256-wide MLP inference kernel (csrc/mlp_infer.hip).

A network is a list of layers, each reading the 256 activations of the previous
layer and/or the per-row INPUT FEATURES (positional encodings).  The input
block can be consumed in two ways:

* as MFMA k-tiles (``w_in``): up to four 32-float tiles, fetched into registers
  by each layer that consumes them, after its activation k-tiles (used by the
  stage-1 networks, whose query points are all distinct);
* as precomputed partial products (``init``): because the layer is linear in
  its input block, W_in [A_row | B_row] = W_a A_row + W_b B_row is evaluated
  ONCE per table row by two small GEMMs and the kernel starts the layer's
  accumulators from U[a] + V[b].  For the stage-2 visibility net the rows are
  all (surface point, light) pairs, so this removes layer 0 and the input half
  of the skip layer from the per-pair work (12 % of the MFMAs).

Dense weights are re-ordered once per optimiser step into MFMA fragment order
by ``psn_mlp_pack_layer``; this module only assembles the zero-padded dense
matrices with torch ops (tiny tensors) and fills the ``PsnMlpDesc``.
"""
import math

import torch

from . import hip


class PackCache(object):
    """The weight packs of one module: ``slot -> pack``, each valid for the parameter values it was built from."""

    def __init__(self):
        self.epoch = 0
        self._slots = {}  # slot -> (key, pack)

    def key(self, params):
        """Cache key of a weight pack: version counter AND storage address of EVERY parameter (an assign-style
        load_state_dict replaces storages of individual layers), plus the invalidation epoch.  In-place edits
        through ``.data`` bump neither: callers that do that (EMA swaps, manual clipping) call ``invalidate_packs()``."""
        return (self.epoch,) + tuple((int(p._version), p.data_ptr()) for p in params)

    def invalidate(self):
        self.epoch += 1

    def get(self, slot, params, build, extra=()):
        """The pack of ``slot`` for the current values of ``params``; ``build(previous pack or None)`` runs (without a graph)
        only when the key changed.  ``extra``: run-time switches that are part of the pack's identity."""
        key = (self.key(params), extra)
        hit = self._slots.get(slot)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                pack = build(hit[1] if hit is not None else None)
            hit = self._slots[slot] = (key, pack)
        return hit[1]


class PackCached(object):
    """Mixin for an nn.Module that runs on weight packs (listed BEFORE nn.Module in the bases): ``self.packs`` and the events
    that invalidate it by themselves -- ``.to()`` / ``.double()`` / ... and ``load_state_dict`` (which visits every submodule
    itself, so every module that owns packs carries the mixin)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.packs = PackCache()

    def invalidate_packs(self):
        """Drop the cached weight packs.  Needed only after editing parameters through ``.data`` (EMA swaps, manual
        clipping): such edits bump neither the version counters nor the storage addresses the caches key on."""
        self.packs.invalidate()

    def _apply(self, fn, *a, **k):
        self.packs.invalidate()
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self.packs.invalidate()
        return super()._load_from_state_dict(*a, **k)


def interleave(weights, biases):
    """[W0, b0, W1, b1, ...]: the parameter order of the autograd functions in ops."""
    return [t for pair in zip(weights, biases) for t in pair]


class PackedMLP(object):
    def __init__(self, desc, w, b, init_wa=None, init_wb=None, init_bias=None):
        self.desc, self.w, self.b = desc, w, b
        # stacked input-block weights of the layers evaluated through init tables
        self.init_wa, self.init_wb, self.init_bias = init_wa, init_wb, init_bias
        self.macs_per_row = None  # algorithmic MACs per row inside the kernel (true, unpadded block shapes)

    def on_points(self, points, pe_octaves, pe_scale, out=None, n_rows_dev=None, out_rows=None, path=None):
        """The network on gamma(pe_scale * points), [Q, 3] -> [Q, n_out], the encoding formed in the kernel prologue
        (hip.mlp_infer_pe): for packs whose input block is one positional encoding and that use no init tables.
        n_rows_dev / out_rows: a compacted list with a device-resident length, outputs scattered; path (see hip.mlp_infer_pe)."""
        return hip.mlp_infer_pe(self.desc, self.w, self.b, points, pe_octaves, pe_scale, out=out, macs_per_row=self.macs_per_row,
                                n_rows_dev=n_rows_dev, out_rows=out_rows, path=path)

    def __call__(self, tab_a, n_rows, a_div=1, a_mod=None, tab_b=None, b_div=1, b_mod=1, *, init_a_direct=None, rank_init=None, **operands):
        """The network on the rows of the index maps; ``operands``: every other keyword of hip.mlp_infer (out, save, mask, live, ...)."""
        if a_mod is None:
            a_mod = tab_a.shape[0] if tab_a is not None else n_rows
        init_a = init_b = None
        if rank_init is not None:
            pass  # the init table as a rank-k product formed inside the kernel (hip.mlp_infer rank_init)
        elif init_a_direct is not None:
            init_a = init_a_direct  # caller-supplied init table (backward chains: d h of the last hidden layer)
        elif self.init_wa is not None:
            # U = A W_a^T (+ bias when there is no B table), V = B W_b^T + bias
            if self.init_wb is None:
                init_a = hip.gemm(tab_a, self.init_wa, trans_b=True, bias=self.init_bias, epi=hip.EPI_BIAS)
            else:
                init_a = hip.gemm(tab_a, self.init_wa, trans_b=True)
                init_b = hip.gemm(tab_b, self.init_wb, trans_b=True, bias=self.init_bias, epi=hip.EPI_BIAS)
        uses_in = any(self.desc.layers[i].n_kt_in > 0 for i in range(self.desc.n_layers))
        return hip.mlp_infer(self.desc, self.w, self.b, tab_a if uses_in else None, a_div, a_mod,
                             tab_b if uses_in else None, b_div, b_mod, n_rows, init_a=init_a, init_b=init_b,
                             macs_per_row=self.macs_per_row, rank_init=rank_init, **operands)


def _pad_cols(w, n):
    return torch.nn.functional.pad(w, (0, n - w.shape[1])) if w.shape[1] < n else w


def _pad_vec(b, n):
    return torch.nn.functional.pad(b, (0, n - b.shape[0])) if b.shape[0] < n else b


_ZEROS = {}


def _zeros(shape, device):
    """Cached constant zeros (never written): the backward chains are re-packed every step and would otherwise pay a
    fill launch per dummy bias / init block."""
    key = (tuple(shape) if not isinstance(shape, int) else (shape,), str(device))
    z = _ZEROS.get(key)
    if z is None:
        z = _ZEROS[key] = torch.zeros(*key[0], device=device)
        if z.is_cuda:
            # shared by every stream from now on (the stage-2 renderer packs on two): the fill must have happened before any of
            # them reads it -- one host wait per distinct size, ever
            torch.cuda.current_stream(z.device).synchronize()
    return z


DIRECT_INIT = 'direct'  # layer spec init_a=DIRECT_INIT: the init table is supplied by the caller at call time (no weights)


class Transposed(object):
    """Marker for pack_layers: use the transpose of ``w`` (backward chains) without materialising it."""

    def __init__(self, w):
        self.w = w.detach()


def _src(w):
    """(matrix, transpose flag, logical rows, logical cols) of a weight block handed to pack_layers."""
    if isinstance(w, Transposed):
        m = w.w
        return m, True, m.shape[1], m.shape[0]
    m = w.detach()
    return m, False, m.shape[0], m.shape[1]


def pack_layers(layers, in_kt_a, in_kt_b, n_out, out_act, device, has_final=True, width=256, reuse=None, x3=False):
    """layers: list of dicts {w_in | init_a/init_b, w_act, bias, act}.
    w_in: [o, <=in_kt*32] consumed as MFMA k-tiles; init_a [o, in_kt_a*32] / init_b [o, in_kt_b*32]: the same
    block evaluated through precomputed tables instead.  Hidden layers have o <= width (zero padded; width = 256 or
    128, one value per network), the final layer o = n_out <= 32 (<= 64 in a 256-wide chain).  w_act / w_in may be any row-major view with unit
    column stride (column slices of a parameter) or Transposed(w): the pack kernel reads them in place and zero-fills
    the padding, so no padded / concatenated / transposed copies are made on the way.
    reuse: the PackedMLP this call site built last time (same network, new parameter values): its zero-padded init-table
    buffers are written in place -- two slice copies per table instead of a pad (fill + copy) per block and a concatenation.
    Only for packs that no launch in flight on ANOTHER stream still reads.
    x3 (experiment; chain launches of the 256-wide networks): the weight blocks as two bf16 planes (hip.W_BF16X2) for the split-bf16
    form of the chain engine; the final layer of a pack with n_out <= 32 stays fp32."""
    assert width in (64, 128, 256) and (not x3 or width == 256)
    hid = width // 32
    kin = in_kt_a + in_kt_b
    desc = hip.PsnMlpDesc()
    desc.n_layers = len(layers)
    desc.n_out, desc.out_act, desc.in_kt_a, desc.in_kt_b = n_out, out_act, in_kt_a, in_kt_b
    desc.w_format = hip.W_BF16X2 if x3 else hip.W_F32
    assert len(layers) <= hip.MAX_LAYERS
    plan, biases = [], []
    init_wa, init_wb, init_bias = [], [], []
    direct_init_off = None
    off = b_off = 0
    for li, L in enumerate(layers):
        last = has_final and li == len(layers) - 1
        n_mt = (2 if n_out > 32 else 1) if last else hid  # final layer: 32 outputs, or 64 (256-wide chain engine only)
        rows = n_mt * 32
        lay = desc.layers[li]
        lay.init_off = -1
        bias = L['bias'].detach().float()
        bias_pad = rows - bias.shape[0]  # zero entries behind the real ones (appended in the concatenation below)
        if isinstance(L.get('init_a'), str) and L['init_a'] == DIRECT_INIT:
            assert not last and not init_wa and direct_init_off is None
            lay.init_off = 0
            direct_init_off = 0
        elif L.get('init_a') is not None:
            assert not last
            lay.init_off = width * len(init_wa)
            init_wa.append(L['init_a'])
            if L.get('init_b') is not None:
                init_wb.append(L['init_b'])
            init_bias.append(_pad_vec(bias, rows))  # folded into the init table
            bias, bias_pad = _zeros(rows, device), 0
        n_kt_in = n_kt_act = 0
        tile = n_mt * 1024  # floats per 32-feature k-tile of this layer
        lay.w_off, lay.b_off = off, b_off
        if L.get('w_act') is not None:  # K order of the packed layer: activation tiles first, input-feature tiles last
            # only the k-tiles that hold real columns (7 of 8 behind the 217-output layer of the stage-1 geometry network);
            # the final layer always takes the full width (its stage layout is fixed)
            n_kt_act = hid - 1 if (not last and hid > 1 and _src(L['w_act'])[3] <= (hid - 1) * 32) else hid
            plan.append((L['w_act'], n_mt, n_kt_act, off))
            off += n_kt_act * tile
        if L.get('w_in') is not None:
            plan.append((L['w_in'], n_mt, kin, off))
            n_kt_in = kin
            off += kin * tile
        biases.append(bias)
        if bias_pad > 0:
            biases.append(_zeros(bias_pad, device))
        lay.n_kt_in, lay.n_kt_act, lay.n_mt, lay.act = n_kt_in, n_kt_act, n_mt, L['act']
        b_off += rows
    w_buf = torch.empty(max(off, 4), device=device, dtype=torch.float32)
    side = []  # (src, dst) copies of the pack's side tables: ONE launch at the end (hip.copy2d_group) when the call site reuses
    is_zero = [bv.data_ptr() == _zeros(bv.shape[0], device).data_ptr() for bv in biases]  # (cached zeros of one size share one tensor)
    n_bias = sum(bv.shape[0] for bv in biases)
    old_b = getattr(reuse, 'b', None)
    if all(is_zero):
        b_buf = _zeros(n_bias, device)  # all-zero biases of a backward chain
    elif old_b is not None and old_b.numel() == n_bias and old_b.device == w_buf.device and getattr(reuse, 'b_zero', None) == is_zero:
        b_buf, o = old_b, 0  # same layout as last time: the zero segments are in place, the others are rewritten
        for bv, z in zip(biases, is_zero):
            if not z:
                side.append((bv, b_buf[o:o + bv.shape[0]]))
            o += bv.shape[0]
    else:
        b_buf = torch.cat(biases).contiguous()
    group = []
    for w, n_mt, k_tiles, o in plan:
        m, tr, r, c = _src(w)
        assert r <= n_mt * 32 and c <= k_tiles * 32, 'pack_layers: block %dx%d does not fit %dx%d' % (r, c, n_mt * 32, k_tiles * 32)
        group.append((m if m.dtype == torch.float32 else m.float(), tr, n_mt, k_tiles, w_buf[o:o + n_mt * k_tiles * 1024],
                      hip.W_BF16X2 if (x3 and n_mt >= 2) else hip.W_F32))
    hip.mlp_pack_layers(group)  # every block of the network in one launch
    desc.init_stride = width * len(init_wa) if direct_init_off is None else width
    if init_wa:
        def stack(blocks, cols, old):  # [len(blocks) * width, cols], zero padded
            shape = (len(blocks) * width, cols)
            buf = old if (old is not None and tuple(old.shape) == shape and old.device == w_buf.device) else torch.zeros(shape, device=device)
            for i, blk in enumerate(blocks):
                assert blk.shape[0] <= width and blk.shape[1] <= cols
                side.append((blk if blk.dtype == torch.float32 else blk.float(), buf[i * width:i * width + blk.shape[0], :blk.shape[1]]))
            return buf
        n_ib = sum(v.shape[0] for v in init_bias)
        old_ib = getattr(reuse, 'init_bias', None)
        if old_ib is not None and old_ib.numel() == n_ib and old_ib.device == w_buf.device:
            ib, o = old_ib, 0
            for v in init_bias:
                side.append((v, ib[o:o + v.shape[0]]))
                o += v.shape[0]
        else:
            ib = torch.cat(init_bias).contiguous()
        pk = PackedMLP(desc, w_buf, b_buf, stack(init_wa, in_kt_a * 32, getattr(reuse, 'init_wa', None)),
                       stack(init_wb, in_kt_b * 32, getattr(reuse, 'init_wb', None)) if init_wb else None, ib)
    else:
        pk = PackedMLP(desc, w_buf, b_buf)
    pk.b_zero = is_zero
    if side:
        side = [(a_.detach().contiguous() if a_.dim() == 1 else a_.detach(), d_) for a_, d_ in side]
        if all(a_.is_cuda for a_, _ in side):
            hip.copy2d_group(side)  # init-table slices + bias segments: one launch (was a slice copy / a concatenation each)
        else:
            for a_, d_ in side:
                d_.copy_(a_)
    pk.macs_per_row = sum(_src(w)[2] * _src(w)[3] for w, _, _, _ in plan)
    return pk


def pack_relu_mlp(weights, biases, din_a, din_b, skip_at, out_act=hip.OUT_NONE, precompute=True, width=256, reuse=None, x3=False):
    """stage2 Network / Normal_Network (stage2/model/renderer.py:17-49) of width 256: ReLU stack, the
    input is concatenated AFTER layer ``skip_at``.  Input row = [table A (din_a real cols, padded to
    a multiple of 32) | table B (din_b)].  precompute=True evaluates the input block of layer 0 and of the
    skip layer through per-row init tables (see module docstring)."""
    ka = (din_a + 31) // 32
    kb = (din_b + 31) // 32 if din_b > 0 else 0

    def split_in(w):  # [o, din_a + din_b] -> [o, (ka+kb)*32] (single table: the slice itself, the packer zero-fills)
        if kb == 0:
            return w[:, :din_a]
        wa = _pad_cols(w[:, :din_a], ka * 32)
        return torch.cat([wa, _pad_cols(w[:, din_a:din_a + din_b], kb * 32)], dim=1)

    def in_block(W):
        if precompute:
            return dict(init_a=W[:, :din_a], init_b=W[:, din_a:din_a + din_b] if kb else None)
        return dict(w_in=split_in(W))

    layers = []
    n = len(weights)
    for li in range(n):
        W, b = weights[li].detach(), biases[li].detach()
        act = hip.ACT_RELU if li < n - 1 else hip.ACT_NONE
        if li == 0:
            layers.append(dict(w_act=None, bias=b, act=act, **in_block(W)))
        elif li - 1 == skip_at:  # input of this layer is cat[y(256), x]
            layers.append(dict(w_act=W[:, :width], bias=b, act=act, **in_block(W[:, width:])))
        else:
            layers.append(dict(w_act=W, bias=b, act=act))
    assert all(L['bias'].shape[0] == width for L in layers[:-1]), 'fused path: every hidden layer must have the given width'
    return pack_layers(layers, ka, kb, weights[-1].shape[0], out_act, weights[0].device, width=width, reuse=reuse, x3=x3)


# --------------------------------------------------------------------------- reduced-precision engines (bf16, split bf16)
# A packer first PLANS its weight stream as a list of pieces in execution order -- (W, permuted, n_ot, ks0, n_ks) = k-steps of a
# matrix view as hip.lowp_pack takes them, or an int n = n zero k-steps of a hidden layer --, then _lowp_stream sizes, allocates and
# fills the buffer from that list: no size is stated apart from the writes that fill it.
def _lowp_net(weights, biases, out_act, skip_at=None, n_out=None):
    """What every packer starts from -> (desc, float32 weights, float32 biases, the final layer's piece, final bias padded to 32).
    The input block is read by layer 0 and by the layer after ``skip_at``; n_out: the leading output rows that are evaluated."""
    n = len(weights)
    Ws, bs = [w.detach().float().contiguous() for w in weights], [b.detach().float() for b in biases]
    n_out = Ws[-1].shape[0] if n_out is None else n_out
    desc = hip.PsnBf16Desc()
    desc.n_hidden, desc.n_out, desc.out_act = n - 1, n_out, out_act
    for li in range(n - 1):
        desc.has_in[li] = int(li == 0 or li - 1 == skip_at)
    fb = torch.zeros(32, device=Ws[0].device)
    fb[:n_out] = bs[-1][:n_out]
    return desc, Ws, bs, (Ws[-1][:n_out], True, 1, 0, 16), fb


def _lowp_stream(pieces, planes, device):
    """The pieces in order as one bfloat16 buffer, + the 56 KB that the last stage request of either engine over-reads."""
    sizes = [(8 * p if isinstance(p, int) else p[2] * p[4]) * planes * 512 for p in pieces]
    buf = torch.zeros(sum(sizes) + 56 * 512, device=device, dtype=torch.bfloat16)
    off = 0
    for p, size in zip(pieces, sizes):
        if not isinstance(p, int):
            hip.lowp_pack(*p, buf[off:off + size], planes=planes)
        off += size
    return buf


def _bias_cols(b):
    """[256] -> the [256, 2] matrix (bf16(b), b - bf16(b)) of a bias k-step of the bf16 engine."""
    hi = b.to(torch.bfloat16).float()
    return torch.stack([hi, b - hi], dim=1).contiguous()


def _in_columns(W, li, din_a, din_b):
    """The table-A and table-B columns of an input layer's weight (layer 0: the whole matrix; later: behind the 256 activations)."""
    c0 = 0 if li == 0 else 256
    return W[:, c0:c0 + din_a], W[:, c0 + din_a:c0 + din_a + din_b]


def _group_tables(desc, Ws, bs, din_a, din_b):
    """Grouped forms: the input layers' table-A and table-B columns, zero-padded to 64, and their biases, stacked in network
    order -> ([n_in * 256, 64], [n_in * 256, 64], [n_in * 256]) fp32."""
    layers = [li for li in range(desc.n_hidden) if desc.has_in[li]]
    init_wa = torch.zeros(len(layers) * 256, 64, device=Ws[0].device)
    init_wb = torch.zeros_like(init_wa)
    for i, li in enumerate(layers):
        init_wa[i * 256:(i + 1) * 256, :din_a], init_wb[i * 256:(i + 1) * 256, :din_b] = _in_columns(Ws[li], li, din_a, din_b)
    return init_wa, init_wb, torch.cat([bs[li] for li in layers]).contiguous()


def _pack_bf16_stream(desc, Ws, bs, final, din_a, din_b, grouped):
    """Weight stream of the bf16 engine (include/psnerf_hip.h, psn_mlp_infer_bf16 / _grouped).  Input block of an input layer:
    4 k-steps of table A and -- two-table form -- 4 of table B; the grouped form has no bias k-step for such a layer."""
    pieces = []
    for li in range(desc.n_hidden):
        block, bias = [], [(_bias_cols(bs[li]), False, 8, 0, 1)]
        if desc.has_in[li]:
            W_a, W_b = _in_columns(Ws[li], li, din_a, din_b)
            block = [(W_a, False, 8, 0, 4)] + ([] if grouped else [(W_b, False, 8, 0, 4) if din_b > 0 else 4])
            bias = [] if grouped else bias
        if li == 0:
            pieces += block + bias
        else:
            W_act = Ws[li][:, :256]
            pieces += [(W_act, True, 8, 0, 8)] + bias + block + [(W_act, True, 8, 8, 8)]
    return _lowp_stream(pieces + [final], 1, Ws[0].device)


class PackedBf16(object):
    """A 256-wide ReLU network packed for the bf16 inference engine (csrc/mlp_infer_bf16.hip)."""

    def __init__(self, desc, w, final_bias):
        self.desc, self.w, self.final_bias = desc, w, final_bias

    def __call__(self, tab_a, n_rows, a_div=1, a_mod=None, tab_b=None, b_div=1, b_mod=1, out=None):
        """tab_a / tab_b: [n, 64] bfloat16 feature tables (the two halves of the input block)."""
        if a_mod is None:
            a_mod = tab_a.shape[0]
        return hip.mlp_infer_bf16(self.desc, self.w, self.final_bias, tab_a, a_div, a_mod, tab_b, b_div, b_mod, n_rows, out=out)


def pack_relu_mlp_bf16(weights, biases, din_a, din_b, skip_at, out_act=hip.OUT_NONE):
    """stage2 Network (stage2/model/renderer.py:34-49) of width 256 for the bf16 engine: the input row is
    [table A (din_a <= 64 real columns) | table B (din_b <= 64)], concatenated again AFTER layer ``skip_at``.
    Weight stream layout: include/psnerf_hip.h (psn_mlp_infer_bf16)."""
    assert len(weights) - 1 <= hip.MAX_LAYERS and din_a <= 64 and din_b <= 64
    assert all(w.shape[0] == 256 for w in weights[:-1]) and weights[-1].shape[0] <= 32
    desc, Ws, bs, final, fb = _lowp_net(weights, biases, out_act, skip_at)
    return PackedBf16(desc, _pack_bf16_stream(desc, Ws, bs, final, din_a, din_b, False), fb)


class PackedBf16Grouped(object):
    """A 256-wide ReLU network packed for the GROUPED form of the bf16 engine (psn_mlp_infer_bf16_grouped): rows
    (g, n) -> g * Ns + n, the input block of a row is [table A row n | group features of g].  The group's part of every
    input layer is folded into a per-group bias in fp32: V[g, i] = W_b,i @ x_g + b_i (one small product per call)."""

    def __init__(self, desc, w, final_bias, wb_t, b_in):
        self.desc, self.w, self.final_bias = desc, w, final_bias
        self.wb_t = wb_t    # [64, n_in * 256] fp32: the table-B columns of the input layers, transposed, zero rows beyond din_b
        self.b_in = b_in    # [n_in * 256] fp32: the biases of the input layers
        self.n_in = b_in.numel() // 256

    def group_bias(self, tab_b):
        """tab_b [n_groups, 64] fp32 group features -> bias k-steps [n_groups * n_in, 4096] bfloat16."""
        V = hip.gemm(tab_b, self.wb_t, bias=self.b_in, epi=hip.EPI_BIAS)  # [n_groups, n_in * 256]
        return hip.lowp_pack_bias(V.view(-1, 256), 2)

    def __call__(self, tab_a, tab_b, out=None):
        """tab_a [Ns, 64] bfloat16, tab_b [n_groups, 64] float32 -> [n_groups * Ns, n_out] (group-major rows)."""
        return hip.mlp_infer_bf16_grouped(self.desc, self.w, self.final_bias, tab_a, self.group_bias(tab_b), tab_b.shape[0], out=out)


def pack_relu_mlp_bf16_grouped(weights, biases, din_a, din_b, skip_at, out_act=hip.OUT_NONE):
    """As pack_relu_mlp_bf16 for the grouped form: the weight stream holds the table-A columns of the input layers only
    (4 k-steps) and no bias k-step for them (include/psnerf_hip.h, psn_mlp_infer_bf16_grouped)."""
    assert len(weights) - 1 <= hip.MAX_LAYERS and din_a <= 64 and 0 < din_b <= 64
    assert all(w.shape[0] == 256 for w in weights[:-1]) and weights[-1].shape[0] <= 32
    desc, Ws, bs, final, fb = _lowp_net(weights, biases, out_act, skip_at)
    _, init_wb, b_in = _group_tables(desc, Ws, bs, din_a, din_b)
    return PackedBf16Grouped(desc, _pack_bf16_stream(desc, Ws, bs, final, din_a, din_b, True), fb, init_wb.t().contiguous(), b_in)


def pack_geo_occupancy(weights, biases, skips, d_pe, x3=False, out_act=hip.OUT_OCC, negate=False):
    """stage1 occupancy-only network (stage1/model/network.py:85-95,124-125): softplus(beta=100)
    stack, before layer l in ``skips`` the input becomes cat[x, pe]/sqrt(2); only output row 0 of the
    last layer is evaluated, followed by sigmoid(-10 x).  Every query point is distinct, so the input
    block stays on the MFMA k-tile path.  ``out_act`` / ``negate``: see pack_geo_logit."""
    ka = (d_pe + 31) // 32
    layers = []
    n = len(weights)
    inv = 1.0 / math.sqrt(2.0)
    for li in range(n):
        W, b = weights[li].detach(), biases[li].detach()
        last = li == n - 1
        act = hip.ACT_NONE if last else hip.ACT_SOFTPLUS100
        if last:
            W, b = W[:1], b[:1]
            if negate:
                W, b = -W, -b
        if li == 0:
            layers.append(dict(w_in=W, w_act=None, bias=b, act=act))
        elif li in skips:
            d_x = W.shape[1] - d_pe
            layers.append(dict(w_in=W[:, d_x:] * inv, w_act=W[:, :d_x] * inv, bias=b, act=act))
        else:
            layers.append(dict(w_in=None, w_act=W, bias=b, act=act))
    return pack_layers(layers, ka, 0, 1, out_act, weights[0].device, x3=x3)


def pack_geo_logit(weights, biases, skips, d_pe):
    """The occupancy network's NEGATED logit (network.py:forward(return_logits=True) = -1 * logit; the value function of the mesh
    extraction, stage1/model/extracting.py:137-155) on the lean engine: pack_geo_occupancy without the final sigmoid, the sign
    folded into the last layer's row and bias (the negation of every product and of the bias negates the rounded sum exactly)."""
    return pack_geo_occupancy(weights, biases, skips, d_pe, out_act=hip.OUT_NONE, negate=True)


def pack_relu_bwd(weights, skip_at, width=256, bits=False, x3=False):
    """Backward (d x) chain of a 256-wide ReLU MLP for the fused kernel: chain layer j computes
    d h_{l-1} = W_l[:, :256]^T d z_l for l = n-1-j (transposed weight packs, no bias), followed by the ReLU mask of
    the forward activation h_{l-1} (PSN_ACT_RELU_MASK, masks supplied at call time) and a dump of d z_{l-1}.
    Chain layer 0 has no weights: it starts from the caller's init table d h_{n-2} = g_out W_{n-1}.
    Returns a PackedMLP whose call needs init_a_direct, mask=[h_{n-2}, ..., h_0], save=[dz_{n-2}, ..., dz_0].
    bits: the masks are the sign-bit words of the forward launch (PSN_ACT_RELU_BITS; hip.mlp_infer save_bits) instead of the
    activations themselves -- 32 bytes per row and layer instead of 4 x width."""
    n = len(weights)
    dev = weights[0].device
    zeros = _zeros(width, dev)
    act = hip.ACT_RELU_BITS if bits else hip.ACT_RELU_MASK
    layers = [dict(init_a=DIRECT_INIT, init_b=None, w_act=None, bias=zeros, act=act)]
    for l in range(n - 2, 0, -1):  # forward layers n-2 .. 1 -> their transposed [in(256), out(256)] blocks
        layers.append(dict(w_act=Transposed(weights[l][:, :width]), bias=zeros, act=act))
    return pack_layers(layers, 1, 0, 0, hip.OUT_NONE, dev, has_final=False, width=width, x3=x3 and width == 256)


# --------------------------------------------------------------------------- stage-1 geometry-field chains
def _t(w):
    return Transposed(w)


def pack_geo_chains(weights, biases, skips, d_pe, x3=False):
    """The four fused chains of ops.GeoFieldFused for the 256-wide softplus geometry network
    (stage1/model/network.py:85-120); ``weights`` are the EFFECTIVE dense matrices with the 1/sqrt(2) of the skip
    layer already folded in.  Returns dict(fwd, sweep, sweep_bwd, value_bwd, value_bwd_nosweep) of PackedMLP.
    The value pass dumps one tensor per layer, the softplus outputs A_l; the consumer chains take them where they need the
    sigmoids s_l and re-form s = 1 - exp(-100 a) in their activation programs (the ACT_*_A codes).
    ``x3`` (experiment, ops.CHAIN_X3): the four chains' matrix work as three bf16 partial products (pack_layers x3)."""
    n = len(weights)
    assert len(skips) == 1 and weights[1].shape[1] == 256 and weights[n - 1].shape[0] == 257
    sk = skips[0]
    dev = weights[0].device
    W = [w.detach() for w in weights]
    b = [x.detach() for x in biases]
    zeros = _zeros(256, dev)
    ka = (d_pe + 31) // 32
    d_a = W[sk].shape[1] - d_pe  # width of the activation part of the skip layer's input (217)

    def fwd_in(l):  # how forward layer l consumes its input
        if l == 0:
            return dict(w_in=W[0], w_act=None)
        if l == sk:
            return dict(w_in=W[l][:, d_a:], w_act=W[l][:, :d_a])
        return dict(w_in=None, w_act=W[l])

    # F1: value pass, dumps a_{l+1}; HEAD = 256 features, final = occupancy logit
    layers = [dict(bias=b[l], act=hip.ACT_SOFTPLUS100, **fwd_in(l)) for l in range(n - 1)]
    layers.append(dict(w_in=None, w_act=W[n - 1][1:], bias=b[n - 1][1:], act=hip.ACT_HEAD))
    layers.append(dict(w_in=None, w_act=W[n - 1][:1], bias=b[n - 1][:1], act=hip.ACT_NONE))
    fwd = pack_layers(layers, ka, 0, 1, hip.OUT_NONE, dev, x3=x3)

    # F2: reverse sweep r_l = (r_{l+1} * s_l) W_l, starting from row 0 of the last layer (init table with one row)
    layers = [dict(init_a=DIRECT_INIT, init_b=None, w_act=None, bias=zeros, act=hip.ACT_MUL_AUX_A)]
    for l in range(n - 2, 0, -1):
        layers.append(dict(w_act=_t(W[l]), bias=zeros, act=hip.ACT_MUL_AUX_A))
    # ... and ends with r_0 = u_0 W_0 (256 -> d_pe encoding columns) as a 64-output FINAL layer: 4 output tiles instead of the 16
    # of a hidden-type layer, the [Q, d_pe] result written densely
    layers.append(dict(w_act=_t(W[0]), bias=_zeros(64, dev), act=hip.ACT_NONE))
    assert 32 < d_pe <= 64
    sweep = pack_layers(layers, ka, 0, d_pe, hip.OUT_NONE, dev, x3=x3)

    # B1: adjoint of the sweep: du_l = dR_l W_l^T ; dR_{l+1} = du_l * s_l ; dS_l = du_l * R_{l+1}
    layers = [dict(bias=zeros, act=hip.ACT_MUL2_A, **fwd_in(l)) for l in range(n - 1)]
    sweep_bwd = pack_layers(layers, ka, 0, 0, hip.OUT_NONE, dev, has_final=False, x3=x3)

    # B2: adjoint of the value pass: da_l = W_l^T dz_l ; dz_{l-1} = s (da + 100 dS (1 - s))   [or s * da without sweep]
    def value_bwd(act):
        ls = [dict(init_a=DIRECT_INIT, init_b=None, w_act=_t(W[n - 1][1:]), bias=zeros, act=act)]
        for l in range(n - 2, 0, -1):
            ls.append(dict(w_act=_t(W[l]), bias=zeros, act=act))
        return pack_layers(ls, ka, 0, 0, hip.OUT_NONE, dev, has_final=False, x3=x3)

    return dict(fwd=fwd, sweep=sweep, sweep_bwd=sweep_bwd, value_bwd=value_bwd(hip.ACT_SOFTPLUS_BWD_A),
                value_bwd_nosweep=value_bwd(hip.ACT_MUL_AUX_A), d_a=d_a)


def pack_app_chains(weights, biases, d_x, x3=False):
    """stage1 appearance network (stage1/model/network.py:98-106, 128-138): ReLU MLP [d_x + 256] -> 256 x (n-1) -> 3
    whose input is cat[x (points, view encoding, normal: d_x <= 64 columns), 256 geometry features].  The features
    enter the first layer as the chain's initial activations (act_init), x as input-feature k-tiles.
    Returns dict(fwd, bwd): fwd dumps the hidden activations, bwd = ReLU backward chain over transposed packs that
    ends with a HEAD layer producing d features and a 3-output final layer producing d normal."""
    n = len(weights)
    dev = weights[0].device
    W = [w.detach() for w in weights]
    b = [x.detach() for x in biases]
    assert W[0].shape[1] == d_x + 256 and all(w.shape == (256, 256) for w in W[1:n - 1]) and d_x <= 64
    ka = (d_x + 31) // 32
    zeros = _zeros(256, dev)
    layers = [dict(w_in=W[0][:, :d_x], w_act=W[0][:, d_x:], bias=b[0], act=hip.ACT_RELU)]
    for l in range(1, n - 1):
        layers.append(dict(w_in=None, w_act=W[l], bias=b[l], act=hip.ACT_RELU))
    layers.append(dict(w_in=None, w_act=W[n - 1], bias=b[n - 1], act=hip.ACT_NONE))
    # (x3: the backward chain only -- it is linear in its operand once the ReLU masks are fixed; a forward pass with 1e-5 errors
    #  flips the units that sit at their kink and the first layers' gradients then differ by 2e-3 of their scale: measured)
    fwd = pack_layers(layers, ka, 0, W[n - 1].shape[0], hip.OUT_NONE, dev)
    ls = [dict(init_a=DIRECT_INIT, init_b=None, w_act=None, bias=zeros, act=hip.ACT_RELU_MASK)]
    for l in range(n - 2, 0, -1):
        ls.append(dict(w_act=_t(W[l]), bias=zeros, act=hip.ACT_RELU_MASK))
    ls.append(dict(w_act=_t(W[0][:, d_x:]), bias=zeros, act=hip.ACT_HEAD))
    # final layer of the backward chain: d normal = d z_0 W_0[:, d_x-3:d_x] (the HEAD layer leaves d z_0 in the
    # activation registers), so the [Q, 256] x [256, 3] product needs no pass over the dumped d z_0
    ls.append(dict(w_act=_t(W[0][:, d_x - 3:d_x]), bias=_zeros(32, dev), act=hip.ACT_NONE))
    bwd = pack_layers(ls, ka, 0, 3, hip.OUT_NONE, dev, x3=x3)
    return dict(fwd=fwd, bwd=bwd)


class PackedX3Grouped(object):
    """A 256-wide ReLU network packed for the split-bf16 ("bf16x6") engine (csrc/mlp_infer_x3.hip; experiment): rows
    (g, n) -> g * Ns + n, input block [table A row n | group features of g].  As in the exact-fp32 engine the layers that read
    the input block start from the fp32 init tables U[n] = W_a x_n and V[g] = W_b x_g + b (two small GEMMs per call)."""

    def __init__(self, desc, w, bias_steps, final_bias, init_wa, init_wb, init_bias, macs_per_row):
        self.desc, self.w, self.bias_steps, self.final_bias = desc, w, bias_steps, final_bias
        self.init_wa, self.init_wb, self.init_bias = init_wa, init_wb, init_bias
        self.macs_per_row = macs_per_row  # the reference network's MACs per row (what an fp32 evaluation multiplies)

    def __call__(self, tab_a, tab_b, out=None):
        """tab_a [Ns, 64] fp32, tab_b [n_groups, 64] fp32 -> [n_groups * Ns, n_out] fp32 (group-major rows)."""
        U = hip.gemm(tab_a, self.init_wa, trans_b=True)
        V = hip.gemm(tab_b, self.init_wb, trans_b=True, bias=self.init_bias, epi=hip.EPI_BIAS)
        return hip.mlp_infer_x3_grouped(self.desc, self.w, self.bias_steps, self.final_bias, U, V, out=out, macs_per_row=self.macs_per_row)


class PackedX3Occ(object):
    """The stage-1 occupancy network packed for the split-bf16 engine (csrc/mlp_infer_x3.hip, OCC variant; opt-in experiment for
    GRADIENT-FREE queries: shadow rays, ray march, root finder inputs).  Same call surface as PackedMLP.on_points."""

    def __init__(self, desc, w, bias_steps, final_bias, skip_layer, pe_first, macs_per_row):
        self.desc, self.w, self.bias_steps, self.final_bias = desc, w, bias_steps, final_bias
        self.skip_layer, self.pe_first, self.macs_per_row = skip_layer, pe_first, macs_per_row

    def march_sweep(self, origin, direction, far, u, omu, near, n_steps, tau, pe_octaves, pe_scale, early_exit=True):
        """The ray-march sweep (hip.march_sweep_x3): points generated and encoded in the kernel, 128-step blocks with early exit."""
        return hip.march_sweep_x3(self.desc, self.w, self.bias_steps, self.final_bias, origin, direction, far, u, omu, near, n_steps, tau,
                                  pe_octaves, pe_scale, self.skip_layer, self.pe_first, early_exit=early_exit, macs_per_row=self.macs_per_row)

    def on_points(self, points, pe_octaves, pe_scale, out=None, n_rows_dev=None, out_rows=None):
        return hip.mlp_infer_x3_occ(self.desc, self.w, self.bias_steps, self.final_bias, points, pe_octaves, pe_scale,
                                    self.skip_layer, self.pe_first, out=out, n_rows_dev=n_rows_dev, out_rows=out_rows,
                                    macs_per_row=self.macs_per_row)


def _pack_x3(desc, Ws, bs, final, first, bias_layers):
    """Weight stream and bias k-steps of the split-bf16 engine -> (w, bias_steps [n_hidden, 4096], MACs per row of the network):
    ``first`` (layer 0's pieces), every further hidden layer as 16 permuted k-steps, the final layer as one stage; the hidden
    layers in ``bias_layers`` get their bias k-step (rows zero-extended to 256), the others a zero one."""
    B = torch.zeros(desc.n_hidden, 256, device=Ws[0].device)
    for li in bias_layers:
        B[li, :bs[li].numel()] = bs[li]
    w = _lowp_stream(first + [(W[:, :256], True, 8, 0, 16) for W in Ws[1:-1]] + [final], 3, Ws[0].device)
    macs = sum(W.shape[0] * W.shape[1] for W in Ws[:-1]) + desc.n_out * Ws[-1].shape[1]
    return w, hip.lowp_pack_bias(B, 3), macs


def pack_geo_occupancy_x3(weights, biases, skips, d_pe):
    """stage1 occupancy-only network (stage1/model/network.py:85-95,124-125; same arguments as pack_geo_occupancy) for the
    split-bf16 engine.  Weight stream in execution order: layer 0 = 4 natural-order k-steps of the encoding columns (two 48 KB
    stages), every further hidden layer 16 permuted k-steps, the final layer's output row 0 as one stage; every hidden layer
    has a bias k-step.  The skip layer (input cat[h, pe] / sqrt(2)) is an ordinary 256-input layer: its encoding columns are
    input features pe_first .. pe_first + d_pe - 1, which the kernel fills in (1 / sqrt(2) folded into the weights here)."""
    n = len(weights)
    assert len(skips) <= 1 and d_pe <= 48 and 3 <= n <= hip.MAX_LAYERS + 1
    assert all(w.shape[0] <= 256 for w in weights[:-1]) and weights[0].shape[1] == d_pe
    desc, Ws, bs, final, fb = _lowp_net(weights, biases, hip.OUT_OCC, n_out=1)
    skip_layer, pe_first = -1, 0
    for li in skips:
        if 0 < li < n - 1:
            assert Ws[li].shape[1] == 256, 'the skip layer reads cat[h, pe]: 256 input features'
            Ws[li] = Ws[li] * (1.0 / math.sqrt(2.0))
            skip_layer, pe_first = li, 256 - d_pe
    w, bias_steps, macs = _pack_x3(desc, Ws, bs, final, [(Ws[0], False, 8, 0, 4)], range(n - 1))
    return PackedX3Occ(desc, w, bias_steps, fb, skip_layer, pe_first, macs)


def pack_relu_mlp_x3_grouped(weights, biases, din_a, din_b, skip_at, out_act=hip.OUT_NONE):
    """stage2 Network (stage2/model/renderer.py:34-49) of width 256 for the split-bf16 engine, grouped form.  Weight stream in
    execution order (include/psnerf_hip.h, psn_mlp_infer_x3_grouped)."""
    n = len(weights)
    assert 3 <= n <= hip.MAX_LAYERS + 1 and din_a <= 64 and 0 < din_b <= 64
    assert all(w.shape[0] == 256 for w in weights[:-1]) and weights[-1].shape[0] <= 32
    desc, Ws, bs, final, fb = _lowp_net(weights, biases, out_act, skip_at)
    w, bias_steps, macs = _pack_x3(desc, Ws, bs, final, [], [li for li in range(n - 1) if not desc.has_in[li]])
    return PackedX3Grouped(desc, w, bias_steps, fb, *_group_tables(desc, Ws, bs, din_a, din_b), macs)
