"""Case tables and plain-torch definitions for the fused MLP engine (csrc/mlp_infer.hip), launch path by launch path.

Nothing here needs a GPU: tests/test_mlp_cpu.py asserts the coverage of the tables and the quality of the definitions,
tests/test_mlp_gpu.py runs every case on the device.

A *case* is a plain dict.  ``build(case)`` turns it into a network (plain float32 CPU tensors, seeded per case), its
inputs and operands; ``evaluate(net, dtype)`` is the definition of what the launch computes: every layer in the order of
the kernel's header comment, in ``dtype`` (float64 = the truth, float32 = the reference arithmetic), returning the output, the
first and second dump of every hidden layer.  ``dispatch(case)`` restates the conditions of mlp_infer_plan and of the kernel's
prologue in Python: which instantiation runs and in which state every launch switch is.

Weights are randn * 1.2 / sqrt(fan_in), biases randn * 0.05 (the scales of tests/test_kernels_gpu.py).

Family H is the secant root finder (psn_root_find, both forms): ``root_inputs(case)`` builds rays and brackets on the CPU from the
float64 definition, ``root_find_definition`` is the float32 definition of the iterates, ``trace_check`` the float64 check that
follows the kernel's own iterates (teacher-forced: a free-running float64 secant is no truth, a branch on f_mid < 0 may
legitimately flip once f_mid is rounding noise).
"""
import math
import zlib

import numpy as np
import torch

WIDTHS = (64, 128, 256)
MAX_LAYERS = 12            # PSN_MLP_MAX_LAYERS
BLOCK = 64                 # rows per workgroup (4 waves x 16)
RTOL = 1e-5                # helpers.assert_vs_truth(rtol=RTOL, atol='max') per tensor
GUARD = 3                  # guard rows in front of and behind every output / dump buffer
SRC_ROOT = 4               # kSrcRootFp: the feature-parallel root finder's key in the kernel table

# activation programs by name -> PSN_ACT_* (include/psnerf_hip.h; test_mlp_cpu.py compares with the parsed header)
ACT = dict(none=0, relu=1, softplus=2, relu_mask=3, mul_aux=4, mul2=5, softplus_bwd=6, head=7, relu_bits=8,
           mul_aux_a=9, mul2_a=10, softplus_bwd_a=11)
OUT = dict(none=0, sigmoid=1, occ=2)
NEED1 = ('relu_mask', 'mul_aux', 'mul2', 'softplus_bwd', 'relu_bits', 'mul_aux_a', 'mul2_a', 'softplus_bwd_a')
NEED2 = ('mul2', 'softplus_bwd', 'mul2_a', 'softplus_bwd_a')
SECOND = ('softplus', 'mul_aux', 'mul2', 'mul_aux_a', 'mul2_a')
FROM_A = ('mul_aux_a', 'mul2_a', 'softplus_bwd_a')
BASE_MUL = ('mul_aux', 'mul2', 'softplus_bwd')


def case_id(c):
    return c['id']


def _gen(c, salt=0):
    return torch.Generator().manual_seed((zlib.crc32(c['id'].encode()) + 7919 * c.get('seed', 0) + salt) % (2 ** 31))


# --------------------------------------------------------------------------- pack reference (family A)
def pack_reference(W, n_mt, k_tiles, transpose=False):
    """Stage order of mlp_pack_kernel: [kt][e(2)][mt16][lane][4] <- W[16 mt16 + i][32 kt + 16 e + 4 g + c] with lane = 16 g + i,
    W zero-extended to [32 n_mt, 32 k_tiles].  ``transpose``: the memory holds W^T."""
    W = np.asarray(W, dtype=np.float32)
    if transpose:
        W = W.T
    full = np.zeros((32 * n_mt, 32 * k_tiles), dtype=np.float32)
    full[:W.shape[0], :W.shape[1]] = W
    out = np.empty((k_tiles, 2, 2 * n_mt, 64, 4), dtype=np.float32)
    for lane in range(64):
        i, g = lane & 15, lane >> 4
        for e in range(2):
            # rows 16 mt16 + i for every mt16, columns 32 kt + 16 e + 4 g + c for every kt, c
            cols = (32 * np.arange(k_tiles)[:, None] + 16 * e + 4 * g + np.arange(4)[None, :])      # [kt, 4]
            rows = 16 * np.arange(2 * n_mt) + i                                                    # [mt16]
            out[:, e, :, lane, :] = full[rows[None, :, None], cols[:, None, :]]
    return out.reshape(-1)


def _pack_item(name, rows, cols, n_mt, k_tiles, transpose=False, ldw_extra=0, col0=0):
    return dict(id='pack-' + name, rows=rows, cols=cols, n_mt=n_mt, k_tiles=k_tiles, transpose=transpose, ldw_extra=ldw_extra, col0=col0)


# (rows, cols) = the logical block W[rows, cols]; ldw_extra / col0: the block is a column slice of a wider parameter
PACK_ITEMS = [
    _pack_item('ragged217x39', 217, 39, 8, 2),
    _pack_item('3x256-final', 3, 256, 1, 8),
    _pack_item('64x64', 64, 64, 2, 2),
    _pack_item('128x96-into-4x4', 128, 96, 4, 4),
    _pack_item('1x1', 1, 1, 1, 1),
    _pack_item('256x384-full', 256, 384, 8, 12),
    _pack_item('ragged217x39-T', 217, 39, 8, 2, transpose=True),
    _pack_item('39x217-T', 39, 217, 2, 7, transpose=True),
    _pack_item('slice-ldw', 256, 39, 8, 2, ldw_extra=256, col0=256),
    _pack_item('slice-ldw-odd', 100, 63, 4, 2, ldw_extra=5, col0=3),
    _pack_item('slice-ldw-T', 63, 100, 2, 4, transpose=True, ldw_extra=7, col0=2),
]
PACK_GROUP_SIZES = (1, 24, 25)   # PSN_PACK_MAX_ITEMS = 24: 25 items take a second launch


def pack_matrix(item):
    """(storage, view): the float32 parameter and the row-major view of it with unit column stride that is handed to the packer
    (its transpose when item['transpose']); view.shape = (rows, cols) or (cols, rows)."""
    g = _gen(item)
    r, c = (item['cols'], item['rows']) if item['transpose'] else (item['rows'], item['cols'])
    store = torch.randn(r, c + item['ldw_extra'], generator=g)
    return store, store[:, item['col0']:item['col0'] + c]


# --------------------------------------------------------------------------- networks
def _w(g, o, i_cols, fan_in):
    return torch.randn(o, i_cols, generator=g) * (1.2 / math.sqrt(fan_in))


def _b(g, o):
    return torch.randn(o, generator=g) * 0.05


LEAN_DEFAULTS = dict(kind='lean', n=65, width=256, depth=3, act='relu', tiles=(2, 0), mode='kt', n_out=3, out_act='none',
                     skip=1, trim=None, maps=None, save_row0=None, save=None, bits=False, live=None, period=None, orders=(None,),
                     seed=0)


def lean(id_, **kw):
    c = dict(LEAN_DEFAULTS)
    c.update(kw)
    c['id'] = id_
    if c['maps'] is None:
        c['maps'] = (1, c['n'], 1, 1)
    return c


class Net(object):
    """layers: list of dicts {act, Wact, Wa, Wb, bias, mode}; mode in (None, 'kt', 'init', 'direct').  The last entry is the
    final layer when n_out > 0."""

    def __init__(self, c):
        self.c = c
        self.width = c['width']
        self.layers = []
        self.n_out = c['n_out']
        self.out_act = c['out_act']
        self.ka, self.kb = c['tiles']
        # inputs / operands (filled by the builders)
        self.tab_a = self.tab_b = None
        self.maps = c.get('maps') or (1, c['n'], 1, 1)
        self.act_init = None
        self.act_init_rows = None
        self.init_direct = None
        self.rk = None
        self.mask = {}
        self.aux2 = {}

    @property
    def n_hidden(self):
        return len(self.layers) - (1 if self.n_out > 0 else 0)

    def pack_spec(self, to_dev, act_code, direct_marker):
        """Layer dicts for fused.pack_layers."""
        spec = []
        for L in self.layers:
            d = dict(w_act=None if L['Wact'] is None else to_dev(L['Wact']), bias=to_dev(L['bias']), act=act_code(L['act']))
            if L['mode'] == 'kt':
                d['w_in'] = to_dev(L['Wa'] if L['Wb'] is None else torch.cat([L['Wa'], L['Wb']], 1))
            elif L['mode'] == 'init':
                d['init_a'] = to_dev(L['Wa'])
                d['init_b'] = None if L['Wb'] is None else to_dev(L['Wb'])
            elif L['mode'] == 'direct':
                d['init_a'], d['init_b'] = direct_marker, None
            spec.append(d)
        return spec


def build_lean(c):
    """ReLU / softplus / linear stack whose layer 0 and layer ``skip`` read the input block [A row | B row]."""
    g = _gen(c)
    net = Net(c)
    W, (ka, kb), depth = c['width'], c['tiles'], c['depth']
    kin = 32 * (ka + kb)
    prev = 0
    for l in range(depth):
        reads_in = l == 0 or l == c['skip']
        out_dim = W - 39 if (c['trim'] is not None and l == c['trim'] - 1) else W
        fan = prev + (kin if reads_in else 0)
        L = dict(act=c['act'], Wact=_w(g, out_dim, prev, fan) if prev else None, Wa=None, Wb=None, bias=_b(g, out_dim), mode=None)
        if reads_in:
            L['Wa'] = _w(g, out_dim, 32 * ka, fan)
            L['Wb'] = _w(g, out_dim, 32 * kb, fan) if kb else None
            L['mode'] = c['mode']
        net.layers.append(L)
        prev = out_dim
    if c['n_out'] > 0:
        net.layers.append(dict(act='none', Wact=_w(g, c['n_out'], prev, prev), Wa=None, Wb=None, bias=_b(g, c['n_out']), mode=None))
    a_div, a_mod, b_div, b_mod = net.maps
    net.tab_a = torch.randn(a_mod, 32 * ka, generator=g)
    net.tab_b = torch.randn(b_mod, 32 * kb, generator=g) if kb else None
    return net


# ---- positional-encoding prologue (family G)
def pe_columns(xs32, octaves, dtype):
    """[n, 64] encoding of the float32 values xs32 = float32(x * scale): [xs | per octave f: sin(2^f xs) (3), cos(2^f xs) (3)], zero
    padded; 2^f xs is exact in float32, the functions are evaluated in ``dtype``."""
    xs = xs32.to(dtype)
    cols = [xs]
    for f in range(octaves):
        arg = xs * float(2 ** f)
        cols += [torch.sin(arg), torch.cos(arg)]
    out = torch.cat(cols, 1)
    return torch.nn.functional.pad(out, (0, 64 - out.shape[1]))


def sweep_points(origin, direction, far, u, omu, near):
    """psn_sample_points' miss profile in float32, every product and sum rounded separately: d = near omu + far u, p = o + dir d."""
    d = (near * omu)[None, :] + far[:, None] * u[None, :]                       # [N, M]
    return (origin[:, None, :] + direction[:, None, :] * d[:, :, None]).reshape(-1, 3)


def build_pe(c):
    """256-wide occupancy-style network on gamma(scale * p): layer 0 and the skip layer read the 64-column encoding as k-tiles."""
    g = _gen(c)
    net = Net(c)
    d_pe = 3 + 6 * c['octaves']
    depth, skip, kact = c['depth'], c['skip'], c['skip_kact']
    prev = 0
    for l in range(depth):
        reads_in = l == 0 or l == skip
        # 217 outputs -> the next layer reads 7 activation k-tiles: in front of the skip layer (skip_kact = 7: 7 + the encoding), or in
        # front of layer ``trim`` (which need not read the encoding: 7 stages and no input block)
        out_dim = 217 if ((kact == 7 and skip is not None and l == skip - 1) or (c.get('trim') is not None and l == c['trim'] - 1)) else 256
        fan = prev + (d_pe if reads_in else 0)
        L = dict(act=c['act'], Wact=_w(g, out_dim, prev, fan) if prev else None, Wa=None, Wb=None, bias=_b(g, out_dim), mode=None)
        if reads_in:
            L['Wa'] = torch.nn.functional.pad(_w(g, out_dim, d_pe, fan), (0, 64 - d_pe))
            L['mode'] = 'kt'
        net.layers.append(L)
        prev = out_dim
    net.layers.append(dict(act='none', Wact=_w(g, c['n_out'], prev, prev), Wa=None, Wb=None, bias=_b(g, c['n_out']), mode=None))
    if c['src'] == SRC_ROOT:
        net.octaves = c['octaves']
        net.maps = (1, max(c['n'], 1), 1, 1)
        return net          # (the query points are the root finder's own: evaluate(net, dtype, points=...))
    if c['src'] == 3:
        N, M = c['rays'], c['steps']
        o = torch.randn(N, 3, generator=g) * 0.3
        d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
        far = 1.0 + torch.rand(N, generator=g)
        u = torch.linspace(0, 1, M)
        net.sweep = dict(origin=o, direction=d, far=far, u=u, omu=1 - u, near=0.25)
        net.points = sweep_points(o, d, far, u, 1 - u, torch.tensor(0.25))
    else:
        net.points = torch.rand(c['capacity'] if c.get('capacity') else c['n'], 3, generator=g) * 2 - 1
    net.xs32 = net.points * torch.tensor(c['pe_scale'], dtype=torch.float32)   # float32(x * scale)
    net.octaves = c['octaves']
    net.maps = (1, net.points.shape[0], 1, 1)
    return net


# ---- chain programs (family F)
CHAIN_DEFAULTS = dict(kind='chain', n=65, width=256, prog=('relu',), first='kt', n_out=3, out_act='none', tiles=(2, 0), rk=0,
                      direct=False, tile_masks=None, trim=None, act_init_rows=None, seed=0, maps=None,
                      force_chain=False, in_scale=1.0, bits_from_lean=False)


def chain(id_, **kw):
    c = dict(CHAIN_DEFAULTS)
    c.update(kw)
    c['id'] = id_
    c['maps'] = (1, c['n'], 1, 1)
    return c


def a_operand(g, n, W):
    """The dumped softplus output a that the *_A programs read: a < 0 (the encoding half of a skip layer's tile), a = 0, a large."""
    a = torch.rand(n, W, generator=g) * 0.03
    a[:, 0::7] = -torch.rand(n, len(range(0, W, 7)), generator=g)      # cannot come from a softplus: s = 0
    a[:, 3::11] = 0.0
    a[:, 5::13] = 1.0 + torch.rand(n, len(range(5, W, 13)), generator=g)   # s = 1 to float32
    return a


def build_chain(c):
    """first: 'kt' (layer 0 reads table A as k-tiles), 'direct' (layer 0 has no weights: caller's init table and / or rank-k
    init), 'act_init' (layer 0 reads initial activations).  prog: the activation program of every hidden layer."""
    g = _gen(c)
    net = Net(c)
    W, n = c['width'], c['n']
    prev = W if c['first'] == 'act_init' else 0
    for l, act in enumerate(c['prog']):
        out_dim = W - 39 if (c['trim'] is not None and l == c['trim'] - 1) else W
        L = dict(act=act, Wact=None, Wa=None, Wb=None, bias=_b(g, out_dim), mode=None)
        if l == 0 and c['first'] == 'kt':
            L['Wa'], L['mode'] = _w(g, out_dim, 64, 64), 'kt'
        elif l == 0 and c['first'] == 'direct':
            L['mode'], L['bias'] = 'direct', torch.zeros(out_dim)
        else:
            L['Wact'] = _w(g, out_dim, prev, prev)
        net.layers.append(L)
        if act in NEED1:
            if act in FROM_A:
                net.mask[l] = a_operand(g, n, W)
            elif act == 'softplus_bwd':
                net.mask[l] = torch.rand(n, W, generator=g)
            else:
                net.mask[l] = torch.randn(n, W, generator=g)
        if act in NEED2:
            net.aux2[l] = torch.randn(n, W, generator=g) * (0.01 if 'softplus_bwd' in act else 1.0)
        if act != 'head':
            prev = out_dim
    if c['n_out'] > 0:
        net.layers.append(dict(act='none', Wact=_w(g, c['n_out'], prev, prev), Wa=None, Wb=None, bias=_b(g, c['n_out']), mode=None))
    if c['first'] == 'kt':
        net.tab_a = torch.randn(n, 64, generator=g) * c['in_scale']
    if c['first'] == 'act_init':
        rows = n if c['act_init_rows'] is None else c['act_init_rows']
        net.act_init = torch.randn(rows, W, generator=g)
        net.act_init_rows = rows
    if c['first'] == 'direct':
        if c['direct']:
            net.init_direct = torch.randn(n, W, generator=g)
        if c['rk']:
            net.rk = (torch.randn(n, c['rk'], generator=g), torch.randn(c['rk'], W, generator=g))
    return net


def net_from_relu_mlp(weights, biases, din_a, din_b, skip_at, tab_a, tab_b, maps, n, mode='init', out_act='none'):
    """The layers of fused.pack_relu_mlp (stage2/model/renderer.py:17-49) as a Net: the input [A row | B row] enters layer 0 and
    the layer behind ``skip_at``; tables padded to multiples of 32 columns."""
    width = weights[0].shape[0]
    ka, kb = (din_a + 31) // 32, (din_b + 31) // 32
    padc = lambda w, k: torch.nn.functional.pad(w, (0, 32 * k - w.shape[1]))
    net = Net(dict(kind='lean', n=n, width=width, n_out=weights[-1].shape[0], out_act=out_act, tiles=(ka, kb), maps=maps, id='relu-mlp'))
    for li, (Wt, b) in enumerate(zip(weights, biases)):
        last = li == len(weights) - 1
        L = dict(act='none' if last else 'relu', Wact=None, Wa=None, Wb=None, bias=b, mode=None)
        if li == 0 or li - 1 == skip_at:
            Win = Wt if li == 0 else Wt[:, width:]
            L['Wact'] = None if li == 0 else Wt[:, :width]
            L['Wa'], L['Wb'] = padc(Win[:, :din_a], ka), (padc(Win[:, din_a:din_a + din_b], kb) if kb else None)
            L['mode'] = mode
        else:
            L['Wact'] = Wt
        net.layers.append(L)
    net.tab_a, net.tab_b = padc(tab_a, ka), (padc(tab_b, kb) if kb else None)
    return net


def net_from_geo(weights, biases, skips, octaves, points, pe_scale, out_act='occ'):
    """The layers of fused.pack_geo_occupancy (stage1/model/network.py:85-95,124-125) as a Net of kind 'pe': softplus stack, in
    front of a layer in ``skips`` the input becomes cat[x, pe] / sqrt(2); output row 0 of the last layer only."""
    d_pe = 3 + 6 * octaves
    inv = 1.0 / math.sqrt(2.0)
    n = points.shape[0]
    net = Net(dict(kind='pe', src=2, n=n, width=256, n_out=1, out_act=out_act, tiles=(2, 0), maps=(1, n, 1, 1), octaves=octaves,
                   pe_scale=pe_scale, capacity=None, id='geo'))
    padc = lambda w: torch.nn.functional.pad(w, (0, 64 - w.shape[1]))
    for li, (Wt, b) in enumerate(zip(weights, biases)):
        last = li == len(weights) - 1
        L = dict(act='none' if last else 'softplus', Wact=None, Wa=None, Wb=None, bias=b, mode=None)
        if last:
            L['Wact'], L['bias'] = Wt[:1], b[:1]
        elif li == 0:
            L['Wa'], L['mode'] = padc(Wt), 'kt'
        elif li in skips:
            d_x = Wt.shape[1] - d_pe
            L['Wact'], L['Wa'], L['mode'] = Wt[:, :d_x] * inv, padc(Wt[:, d_x:] * inv), 'kt'
        else:
            L['Wact'] = Wt
        net.layers.append(L)
    net.points = points
    net.xs32 = points * torch.tensor(pe_scale, dtype=torch.float32)
    net.octaves = octaves
    return net


def build(c):
    return dict(lean=build_lean, chain=build_chain, pe=build_pe)[c['kind']](c)


# --------------------------------------------------------------------------- the definition
def _sig_from_a(a):
    return 1.0 - torch.exp(-100.0 * torch.clamp(a, min=0.0))


def evaluate(net, dtype, wrong=None, points=None):
    """-> dict(out=[n, n_out] or None, d1=[per hidden layer: first dump], d2=[second dump or None]).
    ``wrong``: one of WRONG_FORMS, a deliberately wrong formulation (test_mlp_cpu.py shows that the bound catches each).
    ``points`` (encoding networks): float32 [n, 3] query points in place of the case's own."""
    c = net.c
    n = c['rays'] * c['steps'] if c.get('src') == 3 else (c.get('capacity') or c['n'])
    xs32 = getattr(net, 'xs32', None)
    if points is not None:
        n, xs32 = points.shape[0], points * torch.tensor(c['pe_scale'], dtype=torch.float32)
    T = lambda t: None if t is None else t.to(dtype)
    rows = torch.arange(n)
    a_div, a_mod, b_div, b_mod = net.maps
    ia = (rows // a_div) % a_mod
    if wrong == 'no_a_div':
        ia = rows % a_mod
    ib = (rows // b_div) % b_mod
    xa = xb = None
    if c['kind'] == 'pe':
        xa = pe_columns(xs32, net.octaves, dtype)
    elif net.tab_a is not None:
        xa = T(net.tab_a)[ia]
        xb = T(net.tab_b)[ib] if net.tab_b is not None else None
    if wrong == 'swap_ab' and xb is not None:         # the A and B blocks of the input row change places
        xa, xb = xb, xa
    xrow = None if xa is None else (xa if xb is None else torch.cat([xa, xb], 1))
    W = net.width
    h = torch.zeros(n, W, dtype=dtype)
    if net.act_init is not None:
        h[:net.act_init_rows] = T(net.act_init)[:net.act_init_rows]
    d1, d2 = [], []
    for l, L in enumerate(net.layers):
        last = net.n_out > 0 and l == len(net.layers) - 1
        o = L['bias'].shape[0]
        z = T(L['bias'])[None, :].expand(n, o).clone()
        if wrong == 'double_bias' and L['mode'] == 'init':
            z = z + T(L['bias'])[None, :]
        if L['Wact'] is not None:
            z = z + h[:, :L['Wact'].shape[1]] @ T(L['Wact']).t()
        if L['mode'] in ('kt', 'init') and not (wrong == 'drop_skip' and l > 0):
            Wrow = T(L['Wa']) if L['Wb'] is None else torch.cat([T(L['Wa']), T(L['Wb'])], 1)
            z = z + xrow[:, :Wrow.shape[1]] @ Wrow.t()
        if L['mode'] == 'direct':
            if net.init_direct is not None:
                z = z + T(net.init_direct)
            if net.rk is not None:
                z = z + T(net.rk[0]) @ T(net.rk[1])
        if last:
            out = z
            if net.out_act == 'sigmoid':
                out = torch.sigmoid(z)
            elif net.out_act == 'occ':
                out = torch.sigmoid(z * (10.0 if wrong == 'occ_sign' else -10.0))
            return dict(out=out, d1=d1, d2=d2)
        # a hidden layer with fewer outputs than the width (217 of 256): zero weight rows and zero bias, z = 0 in the padding
        z = torch.nn.functional.pad(z, (0, W - o))
        act = L['act']
        a1, a2 = T(net.mask.get(l)), T(net.aux2.get(l))
        if act in FROM_A:
            a1, act = _sig_from_a(a1), act[:-2]
        second = None
        if act == 'none':
            a = z
        elif act == 'relu':
            a = torch.relu(z)
        elif act == 'softplus':
            a, second = torch.nn.functional.softplus(z, beta=100), torch.sigmoid(100.0 * z)
        elif act in ('relu_mask', 'relu_bits'):
            a = torch.where(a1 > 0, z, torch.zeros_like(z))
        elif act == 'mul_aux':
            a, second = z * a1, z
        elif act == 'mul2':
            a, second = z * a1, z * a2
        elif act == 'softplus_bwd':
            a = a1 * z + 100.0 * (1.0 - a1) * a2
        elif act == 'head':   # side output: z is dumped, the activations stay
            d1.append(z)
            d2.append(None)
            continue
        else:
            raise KeyError(act)
        d1.append(a)
        d2.append(second)
        h = a
    return dict(out=None, d1=d1, d2=d2)


def checked_tensors(c, res):
    """[(name, tensor)] of an evaluate() result that the GPU test compares with the launch: the output, every first dump and, for
    the chain engine, every second dump (the lean engine has none: its launches dump the post-activation only, so evaluate()'s
    second values of a lean or encoding case are not read).  sigmoid(100 z), the second value of a softplus layer, has a slope of
    25 that multiplies the rounding of z: every chain case with a softplus layer scales its inputs (in_scale) so that the float32
    definition still holds half the bound there."""
    out = [] if res['out'] is None else [('out', res['out'])]
    for l, t in enumerate(res['d1']):
        out.append(('dump%d' % l, t))
    if c['kind'] == 'chain':
        for l, t in enumerate(res['d2']):
            if t is not None:
                out.append(('second%d' % l, t))
    return out


WRONG_FORMS = ('swap_ab', 'no_a_div', 'drop_skip', 'double_bias', 'occ_sign')


def sign_words(dump):
    """Sign-bit words of a dumped activation tensor [n, W] (float32 ndarray): word (row, g) bit 4 mt + r = (feature 16 mt + 4 g + r
    > 0), as int64 [n, 4] (the header of PsnMlpLaunch.save_bits_ptrs)."""
    d = np.asarray(dump)
    n, W = d.shape
    words = np.zeros((n, 4), dtype=np.uint64)
    for mt in range(W // 16):
        for g in range(4):
            for r in range(4):
                words[:, g] |= (d[:, 16 * mt + 4 * g + r] > 0).astype(np.uint64) << np.uint64(4 * mt + r)
    return words.view(np.int64)


# --------------------------------------------------------------------------- dispatch
def layer_shape(net):
    """(n_kt_in, n_kt_act, init) per layer as fused.pack_layers lays them out."""
    hid = net.width // 32
    shapes = []
    for l, L in enumerate(net.layers):
        last = net.n_out > 0 and l == len(net.layers) - 1
        kact = 0
        if L['Wact'] is not None:
            kact = hid - 1 if (not last and hid > 1 and L['Wact'].shape[1] <= (hid - 1) * 32) else hid
        shapes.append((net.ka + net.kb if L['mode'] == 'kt' else 0, kact, L['mode'] in ('init', 'direct')))
    return shapes


def dead_rows(c, live):
    """Rows of a padded launch that are not evaluated (zeros): in every group of ``period`` rows in front of save_row0 the 64-row
    blocks from ceil(live / 64) on."""
    period, row0 = c['period'], c['save_row0']
    rb = min((int(live) + BLOCK - 1) // BLOCK, period // BLOCK)
    dead = np.zeros(c['n'], dtype=bool)
    for g0 in range(0, row0, period):
        dead[g0 + rb * BLOCK:g0 + period] = True
    return dead


def dispatch(c, net=None, point_major=True, live=None, row_parallel=False):
    """The launch path of a case: a restatement of mlp_infer_plan / mlp_infer_pe_impl / psn_march_sweep / psn_root_find and of the
    kernel prologue.  ``row_parallel``: the root finder under PSN_ROOT_FIND_ROW_PARALLEL=1."""
    net = net or build(c)
    hid = net.width // 32
    shapes = layer_shape(net)
    n_layers = len(net.layers)
    n_out = net.n_out
    if c['kind'] == 'pe':
        # (mlp_infer_pe_impl and psn_march_sweep launch ONE instantiation each, unconditionally: nothing to restate but its name)
        if c['src'] == SRC_ROOT:
            # psn_root_find: the feature-parallel kernel, 16 rays per workgroup, or (test hook) the row-parallel engine SRC = 1
            src, per = (1, BLOCK) if row_parallel else (SRC_ROOT, 16)
            return dict(chain=False, hid=8, src=src, trim=True, from_a=False, pair=False, point_major=False, tb='none', half_final=True,
                        wide_final=False, blocks_straddle=False, blocks=(c['n'] + per - 1) // per, name='lean/16/src%d/trim' % src)
        return dict(chain=False, hid=8, src=c['src'], trim=True, from_a=False, pair=False, point_major=False, tb='none',
                    half_final=n_out <= 16, wide_final=False, blocks_straddle=False,
                    name='lean/16/src%d/trim' % c['src'])
    n = c['n']
    acts = [L['act'] for L in net.layers]
    chain_ = (net.act_init is not None or net.rk is not None or c.get('tile_masks') is not None or bool(net.mask) or bool(net.aux2)
                    or any(ACT[a] > ACT['softplus'] for a in acts) or c.get('force_chain', False))
    trim = any(0 < ka_ < hid for _, ka_, _ in shapes)
    from_a = any(a in FROM_A for a in acts)
    a_div, a_mod, b_div, b_mod = net.maps
    has_b = net.tab_b is not None
    blocks = (n + BLOCK - 1) // BLOCK
    pair = (not chain_ and a_div == 1 and has_b and b_div == a_mod and b_div >= BLOCK and 2 <= b_mod < (1 << 20) and n == b_div * b_mod)
    lv = c.get('period') is not None and live is not None
    pm = bool(point_major and pair and (not lv or (c['period'] == b_div and (n - c['save_row0']) % c['period'] == 0)))
    width = net.width
    n_bias = ((n_layers - 1) * width + (64 if n_out > 32 else 32)) if n_out > 0 else n_layers * width
    n_init = sum(1 for s in shapes if s[2])
    init_stride = width * n_init
    init_b = has_b and any(L['mode'] == 'init' for L in net.layers)
    tb = 'none'
    straddle = False
    if init_b and not chain_:
        fits = n_bias + init_stride <= MAX_LAYERS * 256
        # per block: does it straddle two B rows?  (the kernel decides per workgroup; a launch is 'lds' when some block takes LDS)
        firsts = np.arange(blocks) * BLOCK
        lasts = np.minimum(firsts + BLOCK - 1, n - 1)
        same = (firsts // b_div) == (lasts // b_div)     # the same quotient: a wrapped-around equal table row does not count
        straddle = bool((~same).any())
        tb = 'mem-size' if not fits else ('lds' if same.all() else ('mixed' if same.any() else 'mem-straddle'))
    name = '%s/%d%s%s' % ('chain' if chain_ else 'lean', hid * 2, '/trim' if trim else '', '/froma' if from_a else '')
    return dict(chain=chain_, hid=hid, src=0, trim=trim, from_a=from_a, pair=pair, point_major=pm, tb=tb,
                half_final=0 < n_out <= 16, wide_final=chain_ and hid == 8 and n_out > 32, blocks_straddle=straddle, name=name)


# every fp32 entry of the engine's kernel table (kInferKernels), i.e. every instantiation the fp32 dispatcher can launch: mlp_infer_plan,
# mlp_infer_pe_impl, psn_march_sweep and psn_root_find (src4 = the feature-parallel root finder, kSrcRootFp; src1 = the row-parallel one)
INSTANTIATIONS = ('lean/16', 'lean/8', 'lean/4', 'chain/16', 'chain/8', 'chain/4', 'lean/16/trim', 'chain/16/trim',
                  'chain/16/froma', 'chain/16/trim/froma', 'lean/16/src2/trim', 'lean/16/src3/trim', 'lean/16/src4/trim',
                  'lean/16/src1/trim')


# --------------------------------------------------------------------------- case tables
ROWS = (1, 15, 16, 17, 63, 64, 65, 129)
TILES = ((1, 0), (2, 0), (4, 0), (1, 1), (2, 2), (3, 1), (1, 3))

B_CASES = []
# rows x width (ReLU, input as k-tiles with a skip layer; rotating heads)
for i, n_ in enumerate(ROWS):
    for w_ in WIDTHS:
        B_CASES.append(lean('B-rows%d-w%d' % (n_, w_), n=n_, width=w_, n_out=(1, 3, 16, 17, 32)[i % 5],
                            act=('relu', 'softplus', 'none')[(i + w_ // 64) % 3]))
# input tiles, as k-tiles and as init tables (A alone: the bias folded into init_a; A + B: one B row per 16 rows)
for ka_, kb_ in TILES:
    for mode_ in ('kt', 'init'):
        for w_ in ((256, 128) if (ka_, kb_) in ((3, 1), (1, 3), (2, 2)) else (256,)):
            n_ = 65
            B_CASES.append(lean('B-tiles%d+%d-%s-w%d' % (ka_, kb_, mode_, w_), n=n_, width=w_, tiles=(ka_, kb_), mode=mode_,
                                maps=(1, 13, 16, 5) if kb_ else (1, n_, 1, 1)))
# heads
for no_ in (1, 3, 16, 17, 32):
    for oa_ in ('none', 'sigmoid', 'occ'):
        B_CASES.append(lean('B-out%d-%s' % (no_, oa_), n=65, width=(256, 128, 64)[no_ % 3], n_out=no_, out_act=oa_, act='softplus' if oa_ == 'occ' else 'relu'))
# trimmed layer (217 real columns -> 7 activation k-tiles)
B_CASES.append(lean('B-trim217', n=65, trim=2, depth=4, skip=2, act='softplus', n_out=1, out_act='occ'))
B_CASES.append(lean('B-trim217-relu-n129', n=129, trim=1, depth=3, skip=None))
# depth: 10 / 11 / 12 layers with two / two / one init layers -- n_bias + init_stride = 2848 (LDS, the tightest fit of a 256-wide
# network), 3104 and 3104 (both > 12 * 256: memory)
for nl_, skip_ in ((10, 4), (11, 4), (12, None)):
    B_CASES.append(lean('B-depth%d' % nl_, n=128, depth=nl_ - 1, skip=skip_, tiles=(2, 2), mode='init', maps=(1, 64, 64, 2), n_out=1))
B_CASES.append(lean('B-depth5-w64-init', n=129, width=64, depth=4, skip=2, tiles=(1, 1), mode='init', maps=(1, 129, 1, 129)))

# index maps: light-major pairs (a_div, a_mod, b_div, b_mod) = (1, P, P, G), both block orders; point-major rows; a wrapped table
C_CASES = []
for P_, G_ in ((64, 2), (128, 3), (29, 4), (100, 3), (65, 9)):
    for mode_ in ('init', 'kt'):
        C_CASES.append(lean('C-pair-P%d-G%d-%s' % (P_, G_, mode_), n=P_ * G_, maps=(1, P_, P_, G_), tiles=(2, 2), mode=mode_,
                            n_out=1, orders=('row', 'point'), depth=3, skip=1))
C_CASES.append(lean('C-pointmajor-rows', n=3 * 100, maps=(3, 100, 1, 3), tiles=(2, 2), mode='init', n_out=1, orders=('row', 'point')))
# 63 % 7 == 0: the first and the last row of block 0 read the same B row, the rows between them do not
C_CASES.append(lean('C-pointmajor-rows-G7', n=7 * 40, maps=(7, 40, 1, 7), tiles=(2, 1), mode='init', n_out=1, orders=('row', 'point')))
C_CASES.append(lean('C-pointmajor-rows-kt', n=4 * 29, maps=(4, 29, 1, 4), tiles=(3, 1), mode='kt', n_out=3))
C_CASES.append(lean('C-wrapped-table', n=100, maps=(1, 7, 1, 1), tiles=(2, 0), mode='init', n_out=3))
C_CASES.append(lean('C-a_div5-a_mod7', n=100, maps=(5, 7, 1, 1), tiles=(1, 0), mode='kt', n_out=3, width=128))
C_CASES.append(lean('C-a_div3-b_div7', n=129, maps=(3, 50, 7, 19), tiles=(1, 1), mode='init', n_out=2, width=64))

# dumps and sign bits: save_row0 in {0, 1, 16, 17, 48, 64, n - 1} at n in {65, 129}; some save entries None; bits at all widths
D_CASES = []
for n_ in (65, 129):
    for r0_ in sorted({0, 1, 16, 17, 48, 64, n_ - 1}):
        D_CASES.append(lean('D-n%d-row0_%d' % (n_, r0_), n=n_, save_row0=r0_, depth=4, skip=2,
                            save=(True, False, True, True) if r0_ % 2 else (True, True, True, True),
                            act='relu' if r0_ % 3 else 'softplus', bits=r0_ in (0, 17, 64), n_out=1))
for w_ in WIDTHS:
    D_CASES.append(lean('D-bits-w%d' % w_, n=129, width=w_, save_row0=16, depth=3, save=(True, True, True), bits=True))
D_CASES.append(lean('D-bits-some-w128', n=65, width=128, save_row0=0, depth=3, save=(True, False, True), bits=(True, False, False)))

# padded row sets: period x groups x tail; every live count and both block orders inside one case
E_CASES = []
for per_ in (64, 128, 192):
    for gr_ in (1, 3):
        for tail_ in (0, per_, 70):
            n_ = gr_ * per_ + tail_
            bm_ = (n_ + per_ - 1) // per_
            E_CASES.append(lean('E-per%d-g%d-tail%d' % (per_, gr_, tail_), n=n_, period=per_, save_row0=gr_ * per_,
                                maps=(1, per_, per_, bm_), tiles=(2, 2), mode='init', depth=2, skip=None, n_out=1,
                                save=(True, True) if tail_ else None, orders=('row', 'point'),
                                live=(0, 1, 63, 64, 65, per_ - 1, per_, per_ + 5)))

# chain-only features
F_CASES = []
for k_ in (1, 2, 3, 4):
    for dr_ in (False, True):
        F_CASES.append(chain('F-rank%d%s' % (k_, '+direct' if dr_ else ''), n=(1, 63, 65)[k_ % 3], first='direct', rk=k_, direct=dr_,
                             prog=('relu_mask', 'none'), n_out=0, width=256 if k_ != 3 else 128))
for w_ in (256, 128):
    for m_ in (0, 0x0001, 0x8000, 0x00F0, 0xA5A5, 0xFFFF):
        F_CASES.append(chain('F-tiles-w%d-%04x' % (w_, m_), n=65, width=w_, prog=('softplus', 'softplus'), in_scale=0.01, tile_masks=(m_, m_ ^ 0xFFFF if m_ in (0xA5A5, 0x00F0) else m_)))
for no_ in (33, 39, 48, 64):
    F_CASES.append(chain('F-wide%d' % no_, n=(63, 65, 1, 65)[no_ % 4], prog=('relu', 'softplus'), n_out=no_, force_chain=True, in_scale=0.01))
F_CASES.append(chain('F-nout0', n=65, prog=('relu', 'relu'), n_out=0, force_chain=True))
for a_ in ('mul_aux_a', 'mul2_a', 'softplus_bwd_a'):
    F_CASES.append(chain('F-%s' % a_, n=65, prog=('softplus', a_, 'none'), n_out=3, in_scale=0.01))
F_CASES.append(chain('F-froma-trim', n=63, prog=('none', 'mul2_a', 'softplus_bwd_a'), trim=2, n_out=39))
F_CASES.append(chain('F-chain-trim', n=65, prog=('softplus', 'mul_aux', 'relu'), trim=1, n_out=3, in_scale=0.01))
for w_ in WIDTHS:
    F_CASES.append(chain('F-relu_mask-w%d' % w_, n=(65, 63, 1)[w_ // 128], width=w_, prog=('relu_mask', 'relu_mask'), first='kt', n_out=3))
    F_CASES.append(chain('F-act_init-w%d' % w_, n=65, width=w_, prog=('relu_mask', 'none'), first='act_init', n_out=0))
    F_CASES.append(chain('F-act_init_rows-w%d' % w_, n=65, width=w_, prog=('none', 'relu'), first='act_init', act_init_rows=(17, 1, 64)[w_ // 128], n_out=2))
    F_CASES.append(chain('F-relu_bits-w%d' % w_, n=(63, 65, 129)[w_ // 128], width=w_, prog=('relu_bits', 'relu_bits'), first='kt', n_out=0, bits_from_lean=True))
F_CASES.append(chain('F-base-programs-w128', n=63, width=128, prog=('softplus', 'mul_aux', 'mul2', 'head', 'softplus_bwd'), n_out=3, in_scale=0.01))

# encoding prologue
PE_DEFAULTS = dict(kind='pe', src=2, n=65, width=256, depth=4, skip=2, skip_kact=8, trim=None, act='softplus', octaves=6, pe_scale=1.0,
                   n_out=1, out_act='occ', tiles=(2, 0), capacity=None, count=None, scatter=False, seed=0)


def pe(id_, **kw):
    c = dict(PE_DEFAULTS)
    c.update(kw)
    c['id'] = id_
    return c


G_CASES = []
for i, n_ in enumerate(ROWS):
    G_CASES.append(pe('G-rows%d' % n_, n=n_, octaves=(0, 6, 10)[i % 3], pe_scale=(1.0, 0.5, 2.0 / 3.0)[(i // 3) % 3],
                      skip_kact=(7, 8)[i % 2], act=('softplus', 'relu')[(i // 2) % 2]))
for oc_ in (0, 6, 10):
    for sc_ in (1.0, 0.5, 2.0 / 3.0):
        G_CASES.append(pe('G-oct%d-scale%.3f' % (oc_, sc_), n=65, octaves=oc_, pe_scale=sc_, skip_kact=7 if oc_ == 6 else 8,
                          act='relu' if sc_ == 0.5 else 'softplus', n_out=3 if oc_ == 10 else 1, out_act='none' if oc_ == 10 else 'occ'))
for cnt_ in (0, 1, 64, 65, 255, 256):
    for sct_ in (False, True):
        G_CASES.append(pe('G-indirect-count%d%s' % (cnt_, '-scatter' if sct_ else ''), n=cnt_, capacity=256, count=cnt_, scatter=sct_,
                          skip_kact=7 if cnt_ % 2 else 8))
for rays_ in (1, 3):
    for st_ in (64, 192):
        G_CASES.append(pe('G-sweep-rays%d-steps%d' % (rays_, st_), src=3, rays=rays_, steps=st_, n=rays_ * st_, skip_kact=7 if rays_ == 3 else 8))

# --------------------------------------------------------------------------- H: the secant root finder (psn_root_find)
# One small random occupancy network per case.  Rays: 1 .. 129 (16 rays per workgroup in the feature-parallel form, 64 in the
# row-parallel one).  Hidden layers 1, 2, 3, 4, 5, 11: the odd-depth barrier of root_find_fp_kernel, the even depths without it and
# PSN_MLP_MAX_LAYERS.  Stage counts of a layer behind layer 0: 8 activation k-tiles + the encoding (10), 7 + the encoding (9), 7 and
# no input block (``trim``; the odd-count branch followed directly by the prefetch of the next layer), 8 and no input block.
H_N_ITER = (0, 1, 2, 3, 8, 64)    # the iteration counts of the bit-for-bit comparison of the two forms
H_STEPWISE = 8                    # D[0] .. D[8] are compared with the step-by-step composition
H_TRACE = 3                       # D[0] .. D[3] are checked against float64, teacher-forced
H_FAR, H_STEPS = 1.5, 33          # the CPU sweep that finds the brackets: depths linspace(0, H_FAR, H_STEPS)


def root(id_, **kw):
    return pe(id_, src=SRC_ROOT, **kw)


H_CASES = [
    root('H-rays1-depth1', n=1, depth=1, skip=None, octaves=0, pe_scale=1.0, tau=0.5),
    root('H-rays15-depth2-skip8', n=15, depth=2, skip=1, skip_kact=8, act='relu', octaves=6, pe_scale=0.5, tau=0.3),
    root('H-rays16-depth3-skip7-linear', n=16, depth=3, skip=2, skip_kact=7, act='none', octaves=10, pe_scale=2.0 / 3.0, tau=0.5),
    root('H-rays17-depth4-trim', n=17, depth=4, skip=None, trim=2, octaves=6, pe_scale=1.0, tau=0.3),
    root('H-rays63-depth5-skip8', n=63, depth=5, skip=3, skip_kact=8, act='relu', octaves=10, pe_scale=0.5, tau=0.5),
    # (the softplus stack shrinks the signal by 0.72 per layer, so eleven of them leave a logit that the last bias decides; the skip
    #  sits late and the seed is one whose logit changes sign on a third of the unit box -- a choice of inputs, made on the CPU)
    root('H-rays64-depth11-skip7', n=64, depth=11, skip=9, skip_kact=7, octaves=6, pe_scale=2.0 / 3.0, tau=0.5, seed=6),
    root('H-rays65-depth4-skip8', n=65, depth=4, skip=2, skip_kact=8, octaves=6, pe_scale=1.0, tau=0.5),
    root('H-rays129-depth3-skip7', n=129, depth=3, skip=1, skip_kact=7, act='relu', octaves=10, pe_scale=1.0, tau=0.3),
    root('H-rays33-depth1-oct0', n=33, depth=1, skip=None, octaves=0, pe_scale=2.0 / 3.0, tau=0.5),
    root('H-rays65-depth3-trim', n=65, depth=3, skip=None, trim=1, octaves=10, pe_scale=0.5, tau=0.3),
    # (with ReLU and no octaves this network is piecewise linear along a ray: the secant lands on the root in two iterations, f_2 is
    #  rounding noise and the allowance of iterate 3 exceeds the tenth of the bracket -- an unchecked pair, which no case may have)
    root('H-rays17-depth2-trim', n=17, depth=2, skip=None, trim=1, act='relu', octaves=10, pe_scale=1.0, tau=0.5),
]

# the argument checks of psn_root_find (PSN_E_ARG, nothing launched, the output untouched): what is changed on a valid call, and the
# words of the check that must answer
H_ARG_CASES = [
    dict(id='H-ARG-n_iter-1', n_iter=-1, refusal='root_find: n_iter=-1'),
    dict(id='H-ARG-n_iter65', n_iter=65, refusal='root_find: n_iter=65'),
    dict(id='H-ARG-out_act', desc=dict(out_act=OUT['sigmoid']), refusal='expects an occupancy network'),
    dict(id='H-ARG-n_out3', desc=dict(n_out=3), refusal='expects an occupancy network'),
    dict(id='H-ARG-bf16x2', desc=dict(w_format='bf16x2'), refusal='fp32 weight stages only'),
    dict(id='H-ARG-softplus-final', final_act='softplus', refusal='activation'),
    dict(id='H-ARG-in_kt_a1', desc=dict(in_kt_a=1), refusal='the input block is one 64-column positional encoding'),
]


def ray_kinds(n):
    """Per ray: 'x' a genuine crossing bracket, 'benign' the (0, 1, -1, 1) psn_first_crossing writes for a miss, 'dd' d_low == d_high,
    'ff' f_low == f_high (a division by zero: inf, then NaN).  A single ray is a crossing."""
    kinds = []
    for i in range(n):
        kinds.append('x' if n == 1 else 'benign' if i % 16 in (5, 11) else 'dd' if i % 32 == 9 else 'ff' if i % 32 == 25 else 'x')
    return kinds


def secant32(dl, dh, fl, fh):
    """rendering.py:526 in float32, every operation rounded separately: -f_low (d_high - d_low) / (f_high - f_low) + d_low."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return ((-fl) * (dh - dl) / (fh - fl) + dl).astype(np.float32)


def point32(o, v, d):
    """rendering.py:531 in float32: p = ray0 + d_pred * direction, the product rounded before the sum."""
    return (o + (d[:, None] * v).astype(np.float32)).astype(np.float32)


_ROOT = {}


def root_inputs(c):
    """(net, dict(origin [n,3], direction [n,3], bracket [4,n], kinds, tau)) as float32 numpy arrays, built once per process.  The
    brackets of the crossing rays come from the float64 definition: random rays are swept on H_STEPS depths, and a ray whose first
    sample is free yields the pair around its first free -> occupied sign change of occ - tau."""
    if c['id'] in _ROOT:
        return _ROOT[c['id']]
    net = build(c)
    g = _gen(c, salt=1)
    n, tau = c['n'], float(np.float32(c['tau']))
    kinds = ray_kinds(n)
    need = kinds.count('x')
    depths = torch.linspace(0.0, H_FAR, H_STEPS)
    found = []      # (origin, direction, d_low, d_high, f_low, f_high)
    for _ in range(40):
        o = (torch.rand(64, 3, generator=g) * 2 - 1) * 0.6
        v = torch.nn.functional.normalize(torch.randn(64, 3, generator=g), dim=-1)
        p = (o[:, None, :] + v[:, None, :] * depths[None, :, None]).reshape(-1, 3)
        val = evaluate(net, torch.float64, points=p)['out'].reshape(64, H_STEPS) - tau
        change = (val[:, :-1] < 0) & (val[:, 1:] > 0)
        other = (val[:, :-1] * val[:, 1:]) <= 0
        for r in range(64):
            ch = other[r].nonzero().reshape(-1)
            if val[r, 0] < 0 and ch.numel() and bool(change[r, ch[0]]):
                i = int(ch[0])
                found.append((o[r], v[r], depths[i], depths[i + 1], val[r, i].float(), val[r, i + 1].float()))
        if len(found) >= need:
            break
    assert len(found) >= need, '%s: %d of %d crossings found' % (c['id'], len(found), need)
    origin = (torch.rand(n, 3, generator=g) * 2 - 1) * 0.6
    direction = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    bracket = torch.tensor([0.0, 1.0, -1.0, 1.0]).repeat(n, 1)
    it = iter(found)
    for i, k in enumerate(kinds):
        if k == 'x':
            o, v, dl, dh, fl, fh = next(it)
            origin[i], direction[i] = o, v
            bracket[i] = torch.stack([dl, dh, fl, fh])
        elif k == 'dd':
            bracket[i] = torch.tensor([0.4, 0.4, -0.3, 0.2])
        elif k == 'ff':
            bracket[i] = torch.tensor([0.2, 0.7, 0.25, 0.25]) if i % 64 == 25 else torch.tensor([0.2, 0.7, -0.25, -0.25])
    inp = dict(origin=origin.numpy().copy(), direction=direction.numpy().copy(), bracket=bracket.t().contiguous().numpy().copy(),
               kinds=kinds, tau=c['tau'], crossing=np.array([k == 'x' for k in kinds]))
    _ROOT[c['id']] = (net, inp)
    return _ROOT[c['id']]


ROOT_WRONG_FORMS = ('wrong_end', 'tau_plus', 'occ_sign', 'swap_rows', 'one_fewer')


def root_find_definition(net, inp, n_iter, dtype=torch.float32, wrong=None):
    """The definition of psn_root_find: [D[0], .., D[n_iter]] float32 [n], D[k] = the depth after k iterations (rendering.py:525-555:
    the secant estimate of the bracket, then per iteration the occupancy at ray0 + d_pred * direction, the bracket end on its side
    moved, the next estimate).  The network is evaluated in ``dtype``, the secant arithmetic in float32.  ``wrong``: one of
    ROOT_WRONG_FORMS."""
    o, v = inp['origin'], inp['direction']
    dl, dh, fl, fh = (inp['bracket'][r].copy() for r in range(4))
    if wrong == 'swap_rows':
        fl, fh = fh, fl
    tau = np.float32(inp['tau'])
    dp = secant32(dl, dh, fl, fh)
    D = [dp]
    for _ in range(n_iter):
        p = torch.from_numpy(point32(o, v, dp))
        with np.errstate(all='ignore'):
            occ = evaluate(net, dtype, wrong='occ_sign' if wrong == 'occ_sign' else None, points=p)['out'].reshape(-1).float().numpy()
        fm = (occ + tau if wrong == 'tau_plus' else occ - tau).astype(np.float32)
        low = fm < 0
        if wrong == 'wrong_end':
            low = ~low
        dl, fl = np.where(low, dp, dl), np.where(low, fm, fl)
        dh, fh = np.where(low, dh, dp), np.where(low, fh, fm)
        dp = secant32(dl, dh, fl, fh)
        D.append(dp)
    if wrong == 'one_fewer':
        D = [D[0]] + D[:-1]
    return D


def trace_check(net, inp, D):
    """The float64 check of the iterates D[0] .. D[H_TRACE] of the crossing rays, teacher-forced: the state (d_l, d_h, f_l, f_h) is
    float64 with error bounds (beta_l, beta_h) on the two f values, 0 at the start (the kernel reads the bracket exactly).  D[0] must
    have the bits of the float32 formula.  For k = 0, 1, 2: p_k = fl32(o + fl32(D[k] v)) is the kernel's own point, f_k = occ64(p_k) -
    tau, b_k = RTOL |occ64| + RTOL max |occ64| over the case's points of this iterate (the bound family G holds psn_mlp_infer_pe to).
    Moving the low end is admissible if f_k < b_k, the high end if f_k > -b_k; each admissible candidate gives d' = -f_l (d_h - d_l)
    / (f_h - f_l) + d_l with the first-order allowance a' = (|(d_h - d_l) f_h| beta_l + |(d_h - d_l) f_l| beta_h) / (f_h - f_l)^2
    + 4 ulp32(d').  D[k + 1] must lie within a' of an admissible candidate; the state continues with the candidate of the smallest
    |D[k + 1] - d'| / a'.  A pair (ray, k) whose a' exceeds a tenth of the ray's initial bracket width is unchecked.
    -> dict(first_equal, worst = the largest ratio, failures, unchecked, where = (ray, k) of the worst, widest = the largest a' in units
    of the tenth of the bracket width at which a pair counts as unchecked)."""
    sel = inp['crossing']
    o, v = inp['origin'][sel], inp['direction'][sel]
    br = inp['bracket'][:, sel]
    tau = float(np.float32(inp['tau']))
    first = secant32(br[0], br[1], br[2], br[3])
    res = dict(first_equal=bool(np.array_equal(first.view(np.int32), np.asarray(D[0], dtype=np.float32)[sel].view(np.int32))),
               worst=0.0, failures=0, unchecked=0, where=None, widest=0.0)
    dl, dh, fl, fh = (br[r].astype(np.float64) for r in range(4))
    bl, bh = np.zeros_like(dl), np.zeros_like(dl)
    width = dh - dl
    for k in range(H_TRACE):
        dk = np.asarray(D[k], dtype=np.float32)[sel]
        nxt = np.asarray(D[k + 1], dtype=np.float32)[sel].astype(np.float64)
        occ = evaluate(net, torch.float64, points=torch.from_numpy(point32(o, v, dk)))['out'].reshape(-1).numpy()
        fk = occ - tau
        bk = RTOL * np.abs(occ) + RTOL * float(np.abs(occ).max())
        cands = []
        dk64 = dk.astype(np.float64)
        for low, ok in ((True, fk < bk), (False, fk > -bk)):
            cdl, cfl, cbl = (dk64, fk, bk) if low else (dl, fl, bl)
            cdh, cfh, cbh = (dh, fh, bh) if low else (dk64, fk, bk)
            with np.errstate(divide='ignore', invalid='ignore'):
                dn = -cfl * (cdh - cdl) / (cfh - cfl) + cdl
                al = (np.abs((cdh - cdl) * cfh) * cbl + np.abs((cdh - cdl) * cfl) * cbh) / (cfh - cfl) ** 2
                al = al + 4.0 * np.spacing(np.abs(dn).astype(np.float32)).astype(np.float64)
                ratio = np.abs(nxt - dn) / al
            ratio = np.where(ok & np.isfinite(ratio), ratio, np.inf)
            cands.append((ratio, al, (cdl, cdh, cfl, cfh, cbl, cbh)))
        pick_low = cands[0][0] <= cands[1][0]
        ratio = np.where(pick_low, cands[0][0], cands[1][0])
        al = np.where(pick_low, cands[0][1], cands[1][1])
        dl, dh, fl, fh, bl, bh = (np.where(pick_low, a, b) for a, b in zip(cands[0][2], cands[1][2]))
        res['failures'] += int((ratio > 1.0).sum())
        res['unchecked'] += int((al > 0.1 * width).sum())
        res['widest'] = max(res['widest'], float((al / (0.1 * width)).max()) if al.size else 0.0)
        if ratio.size and float(ratio.max()) > res['worst']:
            res['worst'], res['where'] = float(ratio.max()), (int(np.flatnonzero(sel)[int(ratio.argmax())]), k)
    return res


LEAN_CASES = B_CASES + C_CASES + D_CASES
ALL_NET_CASES =B_CASES + C_CASES + D_CASES + E_CASES + F_CASES + G_CASES
SCATTER_ROWS = 300

# the argument checks (PSN_E_ARG, nothing launched)
ARG_CASES = [
    dict(lean('ARG-nout33-lean', n_out=33), refusal='33..64 outputs are built for the 256-wide chain engine only'),
    dict(chain('ARG-nout33-w128', width=128, prog=('relu', 'softplus'), n_out=33, force_chain=True),
         refusal='33..64 outputs are built for the 256-wide chain engine only'),
    dict(chain('ARG-froma-mixed', prog=('softplus', 'mul_aux_a', 'mul_aux'), n_out=3), refusal='do not mix with their base programs'),
    dict(lean('ARG-trim-w128', width=128, trim=1, depth=3, skip=None), refusal='n_kt_act = n_mt - 1 is built for the 256-wide networks only'),
    dict(chain('ARG-final-layer-only', prog=(), first='act_init', n_out=3), refusal='a final layer needs at least one hidden layer'),
]


_REF = {}


def reference(c):
    """(net, float64 result, float32 result) of a case, evaluated once per process and left unchanged."""
    if c['id'] not in _REF:
        net = build(c)
        _REF[c['id']] = (net, evaluate(net, torch.float64), evaluate(net, torch.float32))
    return _REF[c['id']]
