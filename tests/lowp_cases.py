"""Case tables, network builders and CPU references for the reduced-precision inference family: the plain bf16 engine
(csrc/mlp_infer_bf16.hip), the split-bf16 engine (csrc/mlp_infer_x3.hip) and the PSN_W_BF16X2 weight stages of the fp32 engine
(csrc/mlp_infer.hip).

Nothing here needs a GPU: tests/test_lowp_cpu.py asserts the exactness conditions, the coverage of the tables and the
sensitivity of the references, tests/test_lowp_gpu.py runs every case on the device.

The method is that of tests/gemm_cases.py: operands for which the arithmetic is EXACT.  Every product, every partial sum in any
order of accumulation and every rounding to bf16 is representable, so the kernel has to reproduce the float64 result bit for bit,
and a single misplaced element, a dropped bias piece or a wrong rounding mode shows.  The condition that makes a dot product
exact in any order is stated once (``order_free``): all its terms are multiples of one power of two u, and the sum of their
magnitudes stays below 2^24 u -- then every partial sum is an integer multiple of u below 2^24 u, hence a float32.
"""
import math
import zlib

import numpy as np
import torch

NAN_BITS = 0x7FC12345
GUARD = 3
MAX_HIDDEN = 12            # PSN_MLP_MAX_LAYERS
BF_BLOCK, BF_WAVE, BF_TILE = 256, 64, 32      # plain bf16 engine: rows per workgroup / wave / MFMA row tile
X3_BLOCK, X3_WAVE = 128, 32                   # split engine
NO_SKIP = -100
SWAP = (5, 9)              # the two K slots (= features of the previous layer) the 'swap_k' wrong model exchanges


def case_id(c):
    return c['id']


def _gen(c, salt=0):
    return torch.Generator().manual_seed((zlib.crc32(c['id'].encode()) + 7919 * c.get('seed', 0) + salt) % (2 ** 31))


# --------------------------------------------------------------------------- number formats
def bf16(t):
    """Round to nearest even bf16, returned in the dtype of ``t`` (float64 inputs must be float32 values)."""
    if t.dtype == torch.float64:
        assert torch.equal(t.float().double(), t), 'bf16(): the value is not a float32'
    return t.float().to(torch.bfloat16).to(t.dtype)


def bf16_trunc(t):
    """The wrong rounding: truncation of the float32 to its upper 16 bits."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def split3(t32):
    """hi, mid, lo float32: each piece the RNE bf16 of what the previous ones left (x3_split1 / x3_split2)."""
    assert t32.dtype == torch.float32
    hi = bf16(t32)
    r = t32 - hi
    mid = bf16(r)
    lo = bf16(r - mid)
    return hi, mid, lo


def r16(t32):
    """The operand model of a PSN_W_BF16X2 stage: bf16(x) + bf16(x - bf16(x)) (16 significant bits: the sum is exact)."""
    hi = bf16(t32)
    return hi + bf16(t32 - hi)


def pieces_exact_mask(t32):
    """Elementwise: adding the three pieces in float32 in every order gives the operand (a piece that was rounded up into the next
    binade can make hi + lo need 25 bits; such values are rare and the exact cases do not use them as inputs)."""
    p = split3(t32)
    ok = torch.ones_like(t32, dtype=torch.bool)
    for a, b, c in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
        ok = ok & ((p[a] + p[b]) + p[c] == t32) & (p[c] + (p[a] + p[b]) == t32)
    return ok


def pieces_sum_exactly(t32):
    """The premise of the split engine's exact cases, for a whole tensor."""
    return bool(pieces_exact_mask(t32).all())


def lowbit(t):
    """The largest power of two that divides every non-zero element of ``t`` (inf for an all-zero tensor)."""
    t = t.double().reshape(-1)
    t = t[t != 0]
    if t.numel() == 0:
        return math.inf
    m, e = torch.frexp(t)
    mi = (m.abs() * float(2 ** 53)).to(torch.int64)
    low = (mi & -mi).double()
    return float((low * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 53).double())).min())


def order_free(terms, what=''):
    """terms: [(X [n, k], W [o, k]) or (B [.., o],)] of one pre-activation z = sum X W^T + sum B.  Asserts that z is exact in
    float32 whatever the order of accumulation (see the module docstring) and returns it in float64."""
    unit, l1, z = math.inf, 0.0, 0.0
    for t in terms:
        if len(t) == 2:
            X, W = t[0].double(), t[1].double()
            unit = min(unit, lowbit(X) * lowbit(W))
            l1 = l1 + X.abs() @ W.abs().t()
            z = z + X @ W.t()
        else:
            B = t[0].double()
            unit = min(unit, lowbit(B))
            l1 = l1 + B.abs()
            z = z + B
    if torch.is_tensor(l1) and unit < math.inf:
        assert float(l1.max()) < float(2 ** 24) * unit, '%s: partial sums may need more than 24 bits (L1 %.3g, unit %.3g)' % (what, float(l1.max()), unit)
    return z


# --------------------------------------------------------------------------- layout models of the packers (family B3)
def k_index(permuted, ks, h, j):
    """K index of element j of lane half h in k-step ks (header comment of psn_lowp_pack)."""
    if permuted:
        return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3)
    return 16 * ks + 8 * h + j


def pack_source(W, permuted, n_ot, ks0, n_ks, swap=None):
    """[n_ks, n_ot, 64 lanes, 8] float32: the source element of every packed slot, lane (m = lane & 31, h = lane >> 5), element j
    <- W[32 ot + m][k_index(ks0 + ks, h, j)], W zero-extended.  ``swap`` = (a, b): the wrong model with two K slots exchanged."""
    W = np.asarray(W, dtype=np.float32)
    full = np.zeros((32 * n_ot, 256), dtype=np.float32)
    full[:W.shape[0], :W.shape[1]] = W
    lane, j = np.arange(64), np.arange(8)
    m, h = lane & 31, lane >> 5
    k = np.empty((n_ks, 64, 8), dtype=np.int64)
    for ks in range(n_ks):
        k[ks] = k_index(permuted, ks0 + ks, h[:, None], j[None, :])
    if swap is not None:
        a, b = swap
        k = np.where(k == a, b, np.where(k == b, a, k))
    r = 32 * np.arange(n_ot)[:, None] + m[None, :]                       # [ot, lane]
    return full[r[None, :, :, None], k[:, None, :, :]]


def _bits16(t):
    return t.to(torch.bfloat16).contiguous().view(torch.int16).numpy()


def pack_bf16_reference(W, permuted, n_ot, ks0, n_ks):
    """psn_lowp_pack, one plane: every element the RNE bf16 of its source -> int16 bit patterns, flat."""
    return _bits16(torch.from_numpy(pack_source(W, permuted, n_ot, ks0, n_ks))).reshape(-1)


def pack_x3_reference(W, permuted, n_ot, ks0, n_ks):
    """psn_lowp_pack, three planes: [ks][ot][plane][lane][8], plane p = piece p of split3 -> int16 bit patterns, flat."""
    src = torch.from_numpy(pack_source(W, permuted, n_ot, ks0, n_ks))
    return _bits16(torch.stack(split3(src), dim=2)).reshape(-1)


def bias_step_reference(V, n_pieces):
    """Bias k-steps [n][8 tiles][64 lanes][8]: K slot 8 h + j = piece (8 h + j) of V[r, 32 ot + (lane & 31)] for the first
    ``n_pieces`` slots (psn_lowp_pack_bias; 2: hi and bf16(v - hi); 3: hi, mid, lo), every other slot 0."""
    V = torch.as_tensor(V, dtype=torch.float32)
    n = V.shape[0]
    out = torch.zeros(n, 8, 64, 8)
    v = V.reshape(n, 8, 32)
    p = split3(v)
    for i in range(n_pieces):
        out[:, :, :32, i] = p[i]
    return _bits16(out).reshape(-1)


def _pk(name, rows, cols, permuted, n_ot, ks0, n_ks, ldw_extra=0, col0=0):
    return dict(id='pack-' + name, rows=rows, cols=cols, permuted=permuted, n_ot=n_ot, ks0=ks0, n_ks=n_ks, ldw_extra=ldw_extra, col0=col0)


# rows < 32 n_ot and cols < 16 (ks0 + n_ks) in every item but the full one: the zero extension is exercised
PACK_ITEMS = [
    _pk('nat-200x100', 200, 100, False, 8, 0, 8),
    _pk('nat-ks2-31x40-final', 31, 40, False, 1, 2, 2),
    _pk('nat-bias-cols', 256, 2, False, 8, 0, 1),
    _pk('perm-217x250-ks8', 217, 250, True, 8, 8, 8),
    _pk('perm-5x100-final', 5, 100, True, 1, 0, 16),
    _pk('perm-1x1', 1, 1, True, 1, 0, 1),
    _pk('perm-full', 256, 256, True, 8, 0, 16),
    _pk('nat-slice-ldw', 100, 63, False, 8, 0, 4, ldw_extra=67, col0=3),
    _pk('perm-slice-ldw-ks3', 250, 199, True, 8, 3, 10, ldw_extra=5, col0=2),
]


def pack_matrix(item):
    """(storage, view) of a pack item: float32 values with full mantissas over several binades, a few exact bf16 ties among them
    (1 + 2^-8 goes down, 1 + 3 2^-8 goes up under RNE) and a few zeros."""
    g = _gen(item)
    r, c = item['rows'], item['cols'] + item['ldw_extra']
    store = torch.randn(r, c, generator=g) * torch.pow(torch.tensor(2.0), torch.randint(-6, 7, (r, c), generator=g).float())
    flat = store.view(-1)
    flat[0::7] = (1.0 + 2.0 ** -8) * flat[0::7].sign()
    flat[3::11] = (1.0 + 3.0 * 2.0 ** -8) * 4.0
    flat[5::13] = 0.0
    return store, store[:, item['col0']:item['col0'] + item['cols']]


BIAS_ROWS = (1, 3, 17)     # rows of the bias k-step packers


def bias_matrix(n):
    g = torch.Generator().manual_seed(100 + n)
    V = torch.randn(n, 256, generator=g) * torch.pow(torch.tensor(2.0), torch.randint(-8, 5, (n, 256), generator=g).float())
    V[:, 0::9] = 2.0 ** -8 + 2.0 ** -17
    V[:, 4::10] = 0.0
    return V


# --------------------------------------------------------------------------- family A: the plain bf16 engine
class Net(object):
    pass


BF_DEFAULTS = dict(form='two', n=65, din=(63, 63), depth=4, skip_at=0, n_out=3, out_act='none', maps=None, rpg=None, groups=None,
                   seed=0, kind='int', lp=None)


def two(id_, **kw):
    """Two-table case: depth = number of linear layers (hidden layers + final), maps = (a_div, a_mod, b_div, b_mod)."""
    c = dict(BF_DEFAULTS)
    c.update(kw)
    c['id'] = id_
    if c['maps'] is None:
        P = min(c['n'], 19)
        c['maps'] = (1, P, P, (c['n'] + P - 1) // P)
    if c['din'][1] == 0:
        c['maps'] = (c['maps'][0], c['maps'][1], 1, 1)
    return c


def grouped(id_, **kw):
    c = dict(BF_DEFAULTS)
    c.update(kw)
    c['id'], c['form'] = id_, 'grouped'
    c['n'] = c['rpg'] * c['groups']
    c['maps'] = (1, c['rpg'], c['rpg'], c['groups'])
    return c


def _has_in(li, skip_at):
    return li == 0 or li - 1 == skip_at


def _int_table(g, rows):
    """[rows, 64] integers in [-4, 4] -- the padding columns too: their packed weights are zero, a correct engine ignores them."""
    return torch.randint(-4, 5, (rows, 64), generator=g).float()


def _fill_padding(t, din):
    """Non-zero entries in the columns behind the real ones."""
    t[:, din:] = torch.where(t[:, din:] == 0, torch.full_like(t[:, din:], 3.0), t[:, din:])
    return t


def build_int_net(c):
    """A1: hidden rows hold one +1 and, with probability 1/2, one -1 at random columns (input block of layer 0 and of the skip
    layer included), hidden biases in {-1, 0, 1, 2}, table entries integers in [-4, 4], final layer dense in {-1, 0, 1} with biases
    k + 0.5: every pre-activation is a small integer."""
    g = _gen(c)
    net = Net()
    net.c = c
    din_a, din_b = c['din']
    din = din_a + din_b
    net.din_a, net.din_b, net.skip_at, net.n_out = din_a, din_b, c['skip_at'], c['n_out']
    depth = c['depth']
    assert 2 <= depth <= MAX_HIDDEN + 1
    Ws, bs = [], []
    for li in range(depth - 1):
        hin = _has_in(li, c['skip_at'])
        F = (0 if li == 0 else 256) + (din if hin else 0)
        W = torch.zeros(256, F)
        c1 = torch.randint(0, F, (256,), generator=g)
        c2 = torch.randint(0, F, (256,), generator=g)
        neg = (torch.rand(256, generator=g) < 0.5) & (c2 != c1)
        W[torch.arange(256), c1] = 1.0
        W[torch.arange(256)[neg], c2[neg]] = -1.0
        if hin:  # the first and the last real column of each table's block are read by some row
            o = F - din
            for r, col in enumerate([o, o + din_a - 1] + ([o + din_a, o + din - 1] if din_b else [])):
                W[r, :] = 0.0
                W[r, col] = 1.0
        Ws.append(W)
        bs.append(torch.randint(-1, 3, (256,), generator=g).float())
    Ws.append(torch.randint(-1, 2, (c['n_out'], 256), generator=g).float())
    Ws[-1][:, SWAP[0]], Ws[-1][:, SWAP[1]] = 1.0, -1.0    # (the two slots of the 'swap_k' model carry different weights)
    bs.append(torch.randint(-2, 3, (c['n_out'],), generator=g).float() + 0.5)
    net.Ws, net.bs = Ws, bs
    a_div, a_mod, b_div, b_mod = c['maps']
    net.tab_a = _fill_padding(_int_table(g, a_mod), din_a)
    net.tab_b = _fill_padding(_int_table(g, b_mod), din_b) if din_b else None
    if net.tab_b is not None and c['form'] == 'grouped':
        net.tab_b[:, din_b:] = 0.0   # (fp32 group features: the binding's contract is zero padding, the GEMM reads all 64 columns)
        net.tab_b[:, 0] = torch.arange(b_mod).float() - 1.0   # every group differs in a column that layer 0 reads
    return net


# ---- A2: rounding probes
P8, P17 = 2.0 ** -8, 2.0 ** -17
# (name, weight on the constant-one source, bias, expected activation): z = w * 1 + bias sits on or next to a bf16 tie
PROBES = [
    ('tie-to-even-down', 0.0, 1.0 + P8, 1.0),                  # RNE 1.0; round-half-up 1 + 2^-7
    ('tie-to-even-up', 0.0, 1.0 + 3 * P8, 1.0 + 2.0 ** -6),    # RNE 1 + 2^-6; truncation 1 + 2^-7
    ('bias-lo-piece', 1.0, P8 + P17, 1.0 + 2.0 ** -7),         # the low bias piece lifts z over the tie; without it: 1.0
    ('above-tie', 1.0, P8 + 2.0 ** -9, 1.0 + 2.0 ** -7),
    ('below-tie', 1.0, 2.0 ** -9, 1.0),
    ('negative', 0.0, -(1.0 + P8), 0.0),
    ('small-negative', 1.0, -1.0 - P8, 0.0),
    ('minus-zero-product', -1.0, 0.0, 0.0),                    # weight -1 on a source that is 0: the product -0 adds nothing (the
    #                                                            sign of a zero cannot be seen in an output: 0 + 0.5 either way)
]
F_ONE, F_GROUP, F_ZERO = 255, 254, 253                         # constant 1 / group-dependent / constant 0 features
PROBE_HIDDEN = 4


def probe_feature(o):
    """Hidden feature read by output o < 31 (probe o % 8): output tile o // 4, spread over the register quads and lane halves."""
    return 8 * o + o % 8


def build_probe_net(c):
    """Four hidden layers; the probes sit in layer c['lp'], features carry over by identity rows, the final layer reads one
    feature per output with weight 1 (one bf16 ulp of a probe = one bf16 ulp of its output).  Two-table form: the probe value is
    the layer's bias (stream bias k-step); grouped form: the probe layer reads the input block, so the value arrives as
    W_b x_g + b through psn_lowp_pack_bias (bf16(b) in the bias, the rest in W_b[:, 0] against x_g[0] = 1)."""
    g = _gen(c)
    net = Net()
    net.c = c
    lp, form = c['lp'], c['form']
    din_a, din_b = c['din']
    din = din_a + din_b
    net.din_a, net.din_b, net.skip_at, net.n_out = din_a, din_b, c['skip_at'], 32
    feats = [probe_feature(o) for o in range(31)]
    assert len(set(feats)) == 31 and max(feats) < F_ZERO
    Ws, bs = [], []
    for li in range(PROBE_HIDDEN):
        hin = _has_in(li, c['skip_at'])
        F = (0 if li == 0 else 256) + (din if hin else 0)
        o_in = F - din
        W, b = torch.zeros(256, F), torch.zeros(256)
        if li == 0:
            b[F_ONE] = 1.0
            W[F_GROUP, din_a + 1] = 1.0     # table B column 1 holds group index + 1
        else:
            W[F_ONE, F_ONE] = 1.0
            W[F_GROUP, F_GROUP] = 1.0
        for o, f in enumerate(feats):
            name, w_one, bias, _ = PROBES[o % 8]
            if li > lp:
                W[f, f] = 1.0
            elif li == lp:
                if w_one != 0.0:
                    if name == 'minus-zero-product':
                        W[f, 2 if li == 0 else F_ZERO] = w_one      # table A column 2 is 0
                    else:
                        W[f, 0 if li == 0 else F_ONE] = w_one       # table A column 0 is 1
                if form == 'grouped':
                    assert hin, 'grouped probes arrive through the group bias: the probe layer reads the input block'
                    hi = float(bf16(torch.tensor(bias)))
                    b[f] = hi
                    W[f, o_in + din_a] = bias - hi                  # x_g[0] = 1
                else:
                    b[f] = bias
        Ws.append(W)
        bs.append(b)
    Wf = torch.zeros(32, 256)
    for o, f in enumerate(feats):
        Wf[o, f] = 1.0
    Wf[31, F_GROUP] = 1.0
    Ws.append(Wf)
    bs.append(torch.full((32,), 0.5))
    net.Ws, net.bs = Ws, bs
    a_div, a_mod, b_div, b_mod = c['maps']
    net.tab_a = _int_table(g, a_mod)
    net.tab_a[:, 0], net.tab_a[:, 2] = 1.0, 0.0
    net.tab_b = torch.zeros(b_mod, 64)
    net.tab_b[:, 0] = 1.0
    net.tab_b[:, 1] = torch.arange(b_mod).float() + 1.0
    return net


def build_bf16(c):
    return build_probe_net(c) if c['kind'] == 'probe' else build_int_net(c)


WRONG_BF16 = ('swap_k', 'no_bias_lo', 'trunc', 'group0_bias', 'clamp_row0')     # the wrong models bf16_reference can state


def bf16_reference(net, wrong=None):
    """float64 statement of what both forms of the plain bf16 engine compute -> dict(logit [n, n_out], acts, V).
    Inputs and weights rounded to bf16 (exact here), bias as bf16(b) + bf16(b - bf16(b)), wide accumulation, post-ReLU
    activations rounded to bf16 RNE, final bias added in fp32.  Grouped form: table-B columns and bias of an input layer enter as
    V[g] = W_b x_g + b, an fp32 product, split like a bias.  With wrong = None the exactness conditions are asserted."""
    c = net.c
    exact = wrong is None
    n = c['n']
    rows = torch.arange(n)
    a_div, a_mod, b_div, b_mod = c['maps']
    rows_a = rows
    if wrong == 'clamp_row0' and n % BF_TILE:
        rows_a = torch.where(rows >= (n // BF_TILE) * BF_TILE, torch.zeros_like(rows), rows)   # the ragged row tile reads row 0
    ia, ib = (rows_a // a_div) % a_mod, (rows_a // b_div) % b_mod
    if c['form'] == 'grouped':
        nl = rows % c['rpg']
        if wrong == 'clamp_row0' and c['rpg'] % BF_TILE:
            nl = torch.where(nl >= (c['rpg'] // BF_TILE) * BF_TILE, torch.zeros_like(nl), nl)
        ia, ib = nl, rows // c['rpg']
    rnd = bf16_trunc if wrong == 'trunc' else bf16
    din_a, din_b = net.din_a, net.din_b
    xa = bf16(net.tab_a).double()[ia]
    xb = None if net.tab_b is None else net.tab_b.double()[ib]
    if xb is not None and c['form'] == 'two':
        xb = bf16(net.tab_b).double()[ib]
    if exact:
        assert torch.equal(bf16(net.tab_a), net.tab_a) and (net.tab_b is None or c['form'] == 'grouped' or torch.equal(bf16(net.tab_b), net.tab_b))
    h, acts, Vs = None, [], []
    nh = len(net.Ws) - 1
    for li in range(nh):
        W, b = net.Ws[li], net.bs[li]
        terms = []
        if li > 0:
            Wact = W[:, :256]
            hh = h
            if wrong == 'swap_k':
                hh = h.clone()
                hh[:, SWAP[0]], hh[:, SWAP[1]] = h[:, SWAP[1]], h[:, SWAP[0]]
            terms.append((hh, bf16(Wact)))
            if exact:
                assert torch.equal(bf16(Wact), Wact)
        bias = b
        if _has_in(li, net.skip_at):
            o = 0 if li == 0 else 256
            Wa = torch.nn.functional.pad(W[:, o:o + din_a], (0, 64 - din_a))
            terms.append((xa, bf16(Wa)))
            if exact:
                assert torch.equal(bf16(Wa), Wa)
            if din_b:
                Wb = torch.nn.functional.pad(W[:, o + din_a:o + din_a + din_b], (0, 64 - din_b))
                if c['form'] == 'grouped':
                    xg = net.tab_b.double()
                    V = order_free([(xg, Wb), (b[None, :],)], 'V of layer %d' % li) if exact else xg @ Wb.double().t() + b.double()
                    if exact:
                        assert torch.equal(V.float().double(), V)
                    Vs.append(V.float())
                    bias = V.float()[torch.zeros_like(ib) if wrong == 'group0_bias' else ib]
                else:
                    terms.append((xb, bf16(Wb)))
                    if exact:
                        assert torch.equal(bf16(Wb), Wb)
        bias = bias.float()
        bhi = bf16(bias)
        terms.append((bhi if bias.dim() == 2 else bhi[None, :],))
        if wrong != 'no_bias_lo':
            blo = bf16(bias - bhi)
            terms.append((blo if bias.dim() == 2 else blo[None, :],))
            if exact:
                assert torch.equal(bhi + blo, bias), 'a bias of layer %d needs more than two bf16 pieces' % li
        if exact:
            z = order_free(terms, '%s layer %d' % (c['id'], li))
        else:
            z = sum((t[0].double() @ t[1].double().t()) if len(t) == 2 else t[0].double() for t in terms)
        a = torch.relu(z)
        if exact:
            assert float(z.abs().max()) <= 256.0
            if c['kind'] == 'int':
                assert torch.equal(bf16(a), a), 'layer %d: an activation is not a bf16' % li
        h = rnd(a.float()).double() if not exact else bf16(a)
        acts.append(h)
    Wf = net.Ws[-1]
    hh = h
    if wrong == 'swap_k':
        hh = h.clone()
        hh[:, SWAP[0]], hh[:, SWAP[1]] = h[:, SWAP[1]], h[:, SWAP[0]]
    if exact:
        assert torch.equal(bf16(Wf), Wf)
        s = order_free([(hh, Wf)], '%s final layer' % c['id'])
        assert torch.equal(s.float().double(), s)
    else:
        s = hh @ bf16(Wf).double().t()
    logit = s + net.bs[-1].double()[None, :]
    if exact:
        assert torch.equal(logit.float().double(), logit), 'an output is not a float32'
    return dict(logit=logit, acts=acts, V=Vs)


def activated(logit64, out_act):
    """(float64 truth, CPU float32 reference arithmetic) of the output activation on the exact logit."""
    l32 = logit64.float()
    if out_act == 'sigmoid':
        return torch.sigmoid(logit64), torch.sigmoid(l32)
    if out_act == 'occ':
        return torch.sigmoid(logit64 * -10.0), torch.sigmoid(l32 * -10.0)
    return logit64, l32


A_ROWS = (1, 31, 32, 33, 64, 65, 255, 256, 257, 513)
A_DIN = ((63, 63), (64, 64), (1, 1), (33, 17), (40, 0))
A_NOUT = (1, 2, 31, 32)
A_DEPTH_SKIP = ((2, NO_SKIP), (5, 0), (5, 2), (4, NO_SKIP), (13, 5))   # one hidden layer; skip at layer 1; at the last hidden
#                                                                        layer (depth - 3); none; the deepest network (12 hidden)
A_RPG, A_GROUPS = (1, 255, 256, 257), (1, 3)

A1_TWO = []
for i_, n_ in enumerate(A_ROWS):
    A1_TWO.append(two('A1-rows%d' % n_, n=n_, n_out=A_NOUT[i_ % 4], depth=(4, 3, 5)[i_ % 3], skip_at=(0, NO_SKIP, 1)[i_ % 3]))
A1_TWO.append(two('A1-map-pair', n=257, maps=(1, 64, 64, 5)))                 # a_div = 1, b_div = a_mod
A1_TWO.append(two('A1-map-adiv5-wrap', n=65, maps=(5, 3, 1, 7)))              # (r // 5) % 3 wraps at r = 15, inside a row tile
A1_TWO.append(two('A1-map-bmod1', n=65, maps=(1, 65, 3, 1)))
A1_TWO.append(two('A1-single-table', n=65, din=(40, 0), maps=(5, 7, 1, 1)))   # tab_b = None, din_b = 0
for da_, db_ in A_DIN:
    A1_TWO.append(two('A1-din%d+%d' % (da_, db_), n=65, din=(da_, db_), skip_at=1))
for d_, s_ in A_DEPTH_SKIP:
    A1_TWO.append(two('A1-depth%d-skip%s' % (d_, 'none' if s_ == NO_SKIP else s_), n=257 if d_ == 13 else 65, depth=d_, skip_at=s_, n_out=2))
for no_ in A_NOUT:
    A1_TWO.append(two('A1-nout%d' % no_, n=33, n_out=no_))
A1_TWO.append(two('A1-sigmoid', n=257, n_out=3, out_act='sigmoid'))
A1_TWO.append(two('A1-occ', n=65, n_out=1, out_act='occ'))

A1_GROUPED = []
for i_, rpg_ in enumerate(A_RPG):
    for gr_ in A_GROUPS:
        A1_GROUPED.append(grouped('A1-grouped-rpg%d-g%d' % (rpg_, gr_), rpg=rpg_, groups=gr_, depth=(4, 5)[i_ % 2], skip_at=(0, 2)[i_ % 2],
                                  n_out=A_NOUT[(i_ + gr_) % 4]))
A1_GROUPED.append(grouped('A1-grouped-deepest', rpg=33, groups=3, depth=13, skip_at=5, n_out=2))
A1_GROUPED.append(grouped('A1-grouped-din33+17', rpg=65, groups=3, din=(33, 17), skip_at=1))
A1_GROUPED.append(grouped('A1-grouped-sigmoid', rpg=257, groups=3, out_act='sigmoid', n_out=3))
A1_GROUPED.append(grouped('A1-grouped-occ', rpg=65, groups=3, out_act='occ', n_out=1))

# probes in layer 0, in a middle layer and in the last hidden layer; two-table: the skip layer is layer 1, the probe layers
# take their bias from the stream; grouped: the probe layer is the skip layer (or layer 0), its bias comes from the group table
A2_CASES = []
for lp_ in (0, 2, 3):
    A2_CASES.append(two('A2-two-layer%d' % lp_, kind='probe', lp=lp_, n=65, depth=PROBE_HIDDEN + 1, skip_at=0, n_out=32, maps=(1, 13, 13, 5)))
    A2_CASES.append(grouped('A2-grouped-layer%d' % lp_, kind='probe', lp=lp_, rpg=33, groups=3, depth=PROBE_HIDDEN + 1,
                            skip_at=0 if lp_ == 0 else lp_ - 1, n_out=32))
A_CASES = A1_TWO + A1_GROUPED + A2_CASES

_REF = {}


def reference_bf16(c):
    """(net, reference) of a family-A case, evaluated once per process and left unchanged."""
    if c['id'] not in _REF:
        net = build_bf16(c)
        _REF[c['id']] = (net, bf16_reference(net))
    return _REF[c['id']]


# --------------------------------------------------------------------------- family B1: the split engine, grouped form
X3_DEFAULTS = dict(rpg=33, groups=3, depth=5, skip_at=1, n_out=3, din=(63, 63), seed=0, n_const=32)


def x3case(id_, **kw):
    c = dict(X3_DEFAULTS)
    c.update(kw)
    c['id'] = id_
    c['n'] = c['rpg'] * c['groups']
    return c


def _full_mantissa(g, *shape, above=None):
    """float32 values with full 24-bit mantissas, both signs, over several binades, whose three bf16 pieces add up to the value in
    every order (pieces_exact_mask; the few draws that do not are drawn again).  above: positive values, ``above`` + |draw|."""
    raw = lambda: torch.randn(*shape, generator=g) * torch.pow(torch.tensor(2.0), torch.randint(-3, 4, shape, generator=g).float())
    draw = raw if above is None else (lambda: raw().abs() + above)
    t = draw()
    for _ in range(8):
        bad = ~pieces_exact_mask(t)
        if not bool(bad.any()):
            break
        t = torch.where(bad, draw(), t)
    assert pieces_sum_exactly(t)
    return t


def _pow2(g, n, p_neg=0.25, e_lo=-1, e_hi=1):
    e = torch.randint(e_lo, e_hi + 1, (n,), generator=g).float()
    s = torch.where(torch.rand(n, generator=g) < p_neg, -1.0, 1.0)
    return s * torch.pow(torch.tensor(2.0), e)


def trace_const(l):
    """Feature that carries the bias of hidden layer l (a constant feature there) through identity-like rows to the final layer."""
    return 8 * l + 3


def trace_group(i):
    """Feature that carries V[g] = w x_g + b of the i-th input layer (a per-group bias with a bias contribution) to the final layer."""
    return 8 * i + 5


def build_x3_net(c):
    """Selection network: every hidden row has a single non-zero weight +-2^e, e in {-1, 0, 1} (in an input layer: one in W_a AND
    one in W_b, i.e. z = U[n] + V[g], ONE fp32 addition; in the skip layer a row selects either an activation or a table column
    pair, never both); hidden biases are zero except for the constant features (zero weight row, bias with a full mantissa);
    the final layer has one +-1 per output.  Output 0 reads a feature that is alive and differs from row to row.  The BIASES are
    observed on purpose: feature trace_const(l) is a constant feature of hidden layer l and is handed on by every later layer
    (weight 2^e on itself), feature trace_group(i) of the i-th input layer has no table-A weight, one table-B weight AND a bias,
    so it is V[g] = w x_g + b (the GEMM's two fp32 operations, mirrored in the reference), handed on likewise; a case with 32
    outputs reads every one of them, a case with 3 outputs those of layer 1 and of the last input layer (net.traced)."""
    g = _gen(c)
    net = Net()
    net.c = c
    din_a, din_b = c['din']
    net.din_a, net.din_b, net.skip_at, net.n_out = din_a, din_b, c['skip_at'], c['n_out']
    depth = c['depth']
    assert 3 <= depth <= MAX_HIDDEN + 1
    net.tab_a = torch.zeros(c['rpg'], 64)
    net.tab_a[:, :din_a] = _full_mantissa(g, c['rpg'], din_a)
    net.tab_b = torch.zeros(c['groups'], 64)
    net.tab_b[:, :din_b] = _full_mantissa(g, c['groups'], din_b)
    Ws, bs = [], []
    ar = torch.arange(256)
    for li in range(depth - 1):
        hin = _has_in(li, c['skip_at'])
        F = (0 if li == 0 else 256) + (din_a + din_b if hin else 0)
        W, b = torch.zeros(256, F), torch.zeros(256)
        const = torch.zeros(256, dtype=torch.bool)
        const[torch.randperm(256, generator=g)[:c['n_const']]] = True
        from_in = torch.ones(256, dtype=torch.bool) if li == 0 else ((torch.rand(256, generator=g) < 0.5) if hin else torch.zeros(256, dtype=torch.bool))
        sel_in, sel_act = from_in & ~const, ~from_in & ~const
        if li > 0:
            W[ar[sel_act], torch.randint(0, 256, (256,), generator=g)[sel_act]] = _pow2(g, 256)[sel_act]
        if hin:
            o = F - din_a - din_b
            W[ar[sel_in], o + torch.randint(0, din_a, (256,), generator=g)[sel_in]] = _pow2(g, 256, 0.5)[sel_in]
            in_b = sel_in if not c.get('single') else sel_in & (torch.rand(256, generator=g) < 0.5)   # single: table A XOR table B
            if c.get('single'):
                W[ar[in_b], o:o + din_a] = 0.0
            W[ar[in_b], o + din_a + torch.randint(0, din_b, (256,), generator=g)[in_b]] = _pow2(g, 256, 0.5)[in_b]
        b[const] = _full_mantissa(g, 256)[const].abs() * torch.where(torch.rand(256, generator=g) < 0.2, -1.0, 1.0)[const]
        if not c.get('single'):
            carry = _pow2(g, 256, 0.0)
            own = _full_mantissa(g, 256, above=0.5)
            grp = _full_mantissa(g, 256, above=256.0)
            in_layers = [l for l in range(li + 1) if _has_in(l, c['skip_at'])]
            for r, origin in [(trace_const(l), l) for l in range(li + 1)] + [(trace_group(i), l) for i, l in enumerate(in_layers)]:
                W[r, :], b[r] = 0.0, 0.0
                const[r] = False
                if origin < li:
                    W[r, r] = carry[r]                                   # handed on (an activation column, also in the skip layer)
                elif r == trace_const(li):
                    b[r] = own[r]
                    const[r] = True
                else:                                                    # this input layer's per-group bias feature
                    W[r, F - din_b + int(torch.randint(0, din_b, (1,), generator=g))] = float(_pow2(g, 1, 0.5)[0])
                    b[r] = grp[r]
        last_const = const
        Ws.append(W)
        bs.append(b)
    net.Ws, net.bs = Ws, bs
    # the final layer reads features that are alive in most rows
    net.Ws = Ws + [torch.zeros(c['n_out'], 256)]
    net.bs = bs + [_full_mantissa(g, c['n_out'])]
    h = x3_reference(net, check=False)['acts'][-1]
    score = (h != 0).sum(0) + 1000 * (h != h[:1]).sum(0)   # alive, and not the same in every row (a chain that ends in a constant)
    score[last_const] = 0
    alive = torch.argsort(score, descending=True, stable=True)[:max(c['n_out'], 40)]
    cols = alive[torch.randperm(alive.numel(), generator=g)[:c['n_out']]]
    nh = depth - 1
    n_in = sum(1 for l in range(nh) if _has_in(l, c['skip_at']))
    net.traced = []
    if not c.get('single'):
        want = [('const', l, trace_const(l)) for l in range(nh)] + [('group', i, trace_group(i)) for i in range(n_in)]
        if c['n_out'] < len(want) + 1:
            want = [('const', 1, trace_const(1)), ('group', n_in - 1, trace_group(n_in - 1))] if c['n_out'] >= 3 else []
        for o, (kind, l, f) in enumerate(want, start=1):
            cols[o] = f
            net.traced.append((o, kind, l))
    net.Ws[-1][torch.arange(c['n_out']), cols] = torch.where(torch.rand(c['n_out'], generator=g) < 0.5, -1.0, 1.0)
    return net


WRONG_X3 = ('no_lo', 'bias_no_lo', 'bias_wrong_layer', 'group0', 'in_idx0')


def x3_reference(net, wrong=None, check=True, bias_scale=None):
    """float64 statement of psn_mlp_infer_x3_grouped on a selection network -> dict(out float64 [n, n_out], acts, U, V): the fp32
    operations of an input layer -- V[g] = (w x_g) + b in the GEMM's epilogue, then U[n] + V[g] in the kernel -- and the final-bias
    addition are mirrored as float32 adds, everything else is exact.  Wrong models: 'no_lo' the activations lose their third plane;
    'bias_no_lo' the stream bias k-steps lose theirs; 'bias_wrong_layer' a stream bias k-step is the previous layer's; 'group0'
    every group starts from V[0]; 'in_idx0' the second input layer starts from the first one's tables.  bias_scale = (layer, factor):
    that hidden layer's bias multiplied (to show which outputs observe it)."""
    c = net.c
    exact = wrong is None and check and bias_scale is None
    n = c['n']
    rows = torch.arange(n)
    ia, ig = rows % c['rpg'], rows // c['rpg']
    din_a, din_b = net.din_a, net.din_b
    xa, xg = net.tab_a.double(), net.tab_b.double()
    h, acts, Us, Vs = None, [], [], []
    for li in range(len(net.Ws) - 1):
        W, b = net.Ws[li].double(), net.bs[li].double()
        if bias_scale is not None and bias_scale[0] == li:
            b = (net.bs[li] * bias_scale[1]).double()
        z = torch.zeros(n, 256, dtype=torch.float64)
        if li > 0:
            hh = h
            if wrong == 'no_lo':
                p = split3(h.float())
                hh = (p[0] + p[1]).double()
            z = hh @ W[:, :256].t()
            if exact:
                assert int((W[:, :256] != 0).sum(1).max()) <= 1
        if _has_in(li, net.skip_at):
            o = 0 if li == 0 else 256
            U = xa[:, :din_a] @ W[:, o:o + din_a].t()
            Vp = xg[:, :din_b] @ W[:, o + din_a:o + din_a + din_b].t()
            if exact:
                assert int((W[:, o:o + din_a] != 0).sum(1).max()) <= 1 and int((W[:, o + din_a:] != 0).sum(1).max()) <= 1
                assert torch.equal(U.float().double(), U) and torch.equal(Vp.float().double(), Vp)
                assert not bool(((W[:, o:] != 0).any(1) & (W[:, :o] != 0).any(1)).any()), 'a skip-layer row reads both blocks'
            V32 = Vp.float() + b.float()[None, :]                 # the GEMM's epilogue: one rounded addition where both are non-zero
            Us.append(U.float())
            Vs.append(V32)
            Ui, Vi = (Us[0], Vs[0]) if wrong == 'in_idx0' else (Us[-1], Vs[-1])
            uv = (Ui[ia] + Vi[torch.zeros_like(ig) if wrong == 'group0' else ig]).double()     # the kernel's rounded addition
            if exact:
                assert not bool(((z != 0) & (uv != 0)).any())     # one of the two summands is zero in every element
            z = z + uv
        else:
            if exact:
                assert not bool(((W != 0).any(1) & (b != 0)).any()), 'a bias next to a weight: the sum would round'
            if wrong == 'bias_wrong_layer':
                b = net.bs[li - 1].double()
            if wrong == 'bias_no_lo':
                p = split3(b.float())
                b = (p[0] + p[1]).double()
            z = z + b[None, :]
        if exact:
            assert torch.equal(z.float().double(), z)
        h = torch.relu(z)
        acts.append(h)
    Wf = net.Ws[-1].double()
    if wrong == 'no_lo':
        p = split3(h.float())
        h = (p[0] + p[1]).double()
    s = h @ Wf.t()
    if exact:
        assert int((Wf != 0).sum(1).max()) == 1 and torch.equal(s.float().double(), s)
    out = (s.float() + net.bs[-1][None, :]).double()
    return dict(out=out, acts=acts, U=Us, V=Vs)


B_RPG, B_GROUPS = (1, 31, 32, 33, 127, 128, 129), (1, 3)
B1_CASES = []
for i_, rpg_ in enumerate(B_RPG):
    for gr_ in B_GROUPS:
        B1_CASES.append(x3case('B1-rpg%d-g%d' % (rpg_, gr_), rpg=rpg_, groups=gr_, depth=(3, 5, 5)[i_ % 3], skip_at=(0, 1, NO_SKIP)[(i_ + gr_) % 3],
                               n_out=(1, 3, 32)[(i_ + gr_) % 3]))
# depth = linear layers: 3 is the packer's minimum, 13 = 12 hidden layers its maximum; 32 outputs: every hidden bias is read
for d_, s_ in ((3, 0), (3, NO_SKIP), (5, 0), (5, 1), (5, NO_SKIP), (12, 0), (12, 5), (12, NO_SKIP), (13, 0), (13, 6), (13, NO_SKIP)):
    B1_CASES.append(x3case('B1-depth%d-skip%s' % (d_, 'none' if s_ == NO_SKIP else s_), rpg=129 if d_ < 13 else 33, groups=3, depth=d_,
                           skip_at=s_, n_out=32))
B1_CASES.append(x3case('B1-din33+17', rpg=33, groups=3, din=(33, 17)))

_REF_X3 = {}


def reference_x3(c):
    if c['id'] not in _REF_X3:
        net = build_x3_net(c)
        _REF_X3[c['id']] = (net, x3_reference(net))
    return _REF_X3[c['id']]


def ulp_distance(got32, ref64):
    """Worst distance of float32 values from float64 references (themselves float32 values here) in units of the reference's ulp."""
    ref32 = ref64.float()
    ulp = torch.maximum((torch.nextafter(ref32.abs(), torch.tensor(math.inf)) - ref32.abs()).double(), torch.tensor(2.0 ** -149, dtype=torch.float64))
    return float(((got32.double() - ref64).abs() / ulp).max()) if got32.numel() else 0.0


# --------------------------------------------------------------------------- family B2: occupancy form and sweep
OCC_OCTAVES, OCC_SCALE, OCC_DPE, OCC_PE_FIRST = 6, 0.5, 39, 217
OCC_ROWS = (0, 1, 31, 32, 33, 127, 128, 129)
OCC_CAPACITY, OCC_COUNTS, OCC_SCATTER_ROWS = 129, (100, 129, 200), 300     # indirect form: count below / at / above the capacity
SWEEP_STEPS, SWEEP_RAYS = (128, 256), (1, 3, 70)
SWEEP_T, SWEEP_NEAR = 0.25, 0.25


def sqrt2_partner():
    """The float32 c with float32(c * (1 / sqrt 2)) == 1, in the arithmetic of fused.pack_geo_occupancy (a float32 tensor times
    the Python float): a skip-layer weight +-2^e c is +-2^e after the fold, so the layer stays a selection layer."""
    inv = 1.0 / math.sqrt(2.0)
    c = torch.tensor([math.sqrt(2.0)], dtype=torch.float32)
    for _ in range(4):
        for cand in (c, torch.nextafter(c, torch.tensor([2.0])), torch.nextafter(c, torch.tensor([0.0]))):
            if float((cand * inv)[0]) == 1.0:
                return float(cand[0])
        c = torch.nextafter(c, torch.tensor([2.0]))
    raise AssertionError('no float32 partner of 1 / sqrt 2')


def occ(id_, **kw):
    c = dict(id=id_, n=33, depth=5, skip=2, sweep=False, n_const=24, seed=0, trace=None)
    c.update(kw)
    return c


def build_occ_net(c):
    """Selection-weight occupancy network (stage-1 layout: softplus stack on gamma(0.5 p), 6 octaves; the layer in front of the
    skip layer has 217 outputs, the skip layer reads cat[h, pe] / sqrt 2 -> pe_first = 217): every hidden row has one weight
    +-2^e and a zero bias, or no weight and a bias with a full mantissa; the final row has one +-1.  sweep: row 0 of every layer
    carries coordinate x with weight 1 and the final layer reads it with -1 and bias SWEEP_T, so that the occupancy crosses 1/2
    at the plane 0.5 x = SWEEP_T whatever the other rows do."""
    g = _gen(c)
    net = Net()
    net.c = c
    depth, skip = c['depth'], c['skip']
    part = sqrt2_partner()
    outs = [256] * (depth - 1)
    outs[skip - 1] = OCC_PE_FIRST
    Ws, bs = [], []
    for li in range(depth - 1):
        F = OCC_DPE if li == 0 else (256 if li == skip else outs[li - 1])
        o = outs[li]
        W, b = torch.zeros(o, F), torch.zeros(o)
        const = torch.zeros(o, dtype=torch.bool)
        const[1 + torch.randperm(o - 1, generator=g)[:c['n_const']]] = True
        col = torch.randint(0, F, (o,), generator=g)
        val = _pow2(g, o, 0.25, -2, 0) * (part if li == skip else 1.0)
        W[torch.arange(o)[~const], col[~const]] = val[~const]
        b[const] = _full_mantissa(g, o)[const] * 0.125
        if c['sweep']:
            W[0, :] = 0.0
            W[0, 0] = part if li == skip else 1.0
        if c['trace'] is not None and li >= c['trace']:      # the bias of layer c['trace'], handed on to the final layer
            T = trace_const(c['trace'])
            W[T, :], b[T] = 0.0, 0.0
            if li == c['trace']:
                b[T] = float(_full_mantissa(g, 1, above=0.05)[0]) * 0.125
            else:
                W[T, T] = part if li == skip else 1.0
        Ws.append(W)
        bs.append(b)
    Ws.append(torch.zeros(1, 256))
    bs.append(_full_mantissa(g, 1) * 0.125)
    net.Ws, net.bs, net.skips = Ws, bs, [skip]
    net.points = torch.rand(max(c['n'], 1), 3, generator=g)[:c['n']] * 2 - 1
    if c['sweep']:
        Ws[-1][0, 0] = -1.0
        bs[-1][0] = SWEEP_T
    else:   # the final row reads a feature that varies from point to point
        from tests import mlp_cases as mc
        probe = torch.rand(64, 3, generator=g) * 2 - 1
        h = mc.evaluate(mc.net_from_geo(Ws, bs, [skip], OCC_OCTAVES, probe, OCC_SCALE), torch.float64)['d1'][-1]
        sign = 1.0 if float(torch.rand(1, generator=g)) < 0.5 else -1.0
        f = int(torch.argsort(h.std(0), descending=True)[int(torch.randint(0, 4, (1,), generator=g))])
        if c['trace'] is not None:
            f = trace_const(c['trace'])
        Ws[-1][0, f] = sign
        # the final bias centres the logits: occupancies away from 0 and 1, where a last-bit change of the logit shows
        bs[-1][0] = -sign * float(bf16(h[:, f].median().float())) + 2.0 ** -6
    return net


B2_POINT_CASES = [occ('B2-points%d' % n_, n=n_) for n_ in OCC_ROWS] + [occ('B2-points129-depth7-skip4', n=129, depth=7, skip=4)]
# one output per network: a network per hidden layer whose output is that layer's bias handed on (layer 0: the first bias k-step
# of the launch, layer 1: the one requested with layer 0's second stage, the skip layer, the last hidden layer)
B2_BIAS_CASES = [occ('B2-bias-layer%d' % l_, n=33, trace=l_) for l_ in range(4)]


def sweep_rays(n_rays, n_steps):
    """Rays along +-x against the plane x = 0.5 (step 0.01 in depth): kind 0 crosses between the last step of a 128-step block and
    the first of the next (256 steps; with 128 steps: between the last two steps), kind 1 starts occupied, kind 2 never crosses,
    kind 3 crosses inside the first block.  -> dict(origin, direction, far, u, omu, near, kind)."""
    kinds = torch.arange(n_rays) % 4
    span = 0.01 * (n_steps - 1)
    o = torch.zeros(n_rays, 3)
    d = torch.zeros(n_rays, 3)
    d[:, 0] = 1.0
    cross = 127.5 if n_steps == 256 else n_steps - 1.5          # the step index at which x = 0.5
    for r in range(n_rays):
        k, j = int(kinds[r]), r // 4
        o[r, 1], o[r, 2] = 0.1 * ((r * 7) % 11 - 5), 0.07 * ((r * 3) % 13 - 6)
        if k == 0:
            o[r, 0] = 0.5 - SWEEP_NEAR - 0.01 * cross
        elif k == 1:
            o[r, 0] = 1.0 + 0.01 * j
        elif k == 2:
            d[r, 0] = -1.0
        else:
            o[r, 0] = 0.5 - SWEEP_NEAR - 0.01 * (30.5 + 3 * j)
    u = torch.linspace(0, 1, n_steps)
    return dict(origin=o, direction=d, far=torch.full((n_rays,), SWEEP_NEAR + span), u=u, omu=1 - u, near=SWEEP_NEAR, kind=kinds)


def first_change(val):
    """Per ray of val [N, M] = occupancy - tau: index i of the first pair (i, i + 1) with a negative product, 0 for a ray that does
    not start in free space (val[0] >= 0), -1 for none; and the 128-step block whose workgroup sees it (-1: none does)."""
    N, M = val.shape
    idx = torch.full((N,), -1, dtype=torch.long)
    blk = torch.full((N,), -1, dtype=torch.long)
    for r in range(N):
        neg = ((val[r, :-1] * val[r, 1:]) < 0).nonzero().reshape(-1)
        if not bool(val[r, 0] < 0):
            idx[r], blk[r] = 0, 0
            continue
        if neg.numel():
            idx[r] = int(neg[0])
        inblock = [int(i) for i in neg if int(i) % 128 != 127]
        if inblock:
            blk[r] = inblock[0] // 128
    return idx, blk


# --------------------------------------------------------------------------- family C: PSN_W_BF16X2 weight stages
def x3dot(X, W, dtype):
    """One multiply of a PSN_W_BF16X2 stage in ``dtype``: both operands as bf16(x) + bf16(x - bf16(x)) of their float32 values, kept
    products hi hi + hi mid + mid hi (csrc/mlp_infer.hip, stage_compute_x3)."""
    x32, w32 = X.float(), W.float()
    xh, wh = bf16(x32), bf16(w32)
    xm, wm = bf16(x32 - xh), bf16(w32 - wh)
    T = lambda t: t.to(dtype)
    return T(xh) @ (T(wh) + T(wm)).t() + T(xm) @ T(wh).t()


def c1case(id_, **kw):
    c = dict(X3_DEFAULTS)
    c.update(dict(single=True, form='lean', precompute=False, order=None, live=None, period=None, save_row0=0, maps=None, depth=4, skip_at=1))
    c.update(kw)
    c['id'] = id_
    if c['maps'] is None:
        P = min(c['n'], 13)
        c['maps'] = (1, P, P, (c['n'] + P - 1) // P)
    c['rpg'], c['groups'] = c['maps'][1], c['maps'][3]
    return c


C1_ROWS = (1, 63, 64, 65, 129)
C1_CASES = [c1case('C1-lean-rows%d' % n_, n=n_, n_out=(1, 3, 32)[i_ % 3]) for i_, n_ in enumerate(C1_ROWS)]
# padded launch: one group of 128 rows in front of save_row0, 33 of them live -> the block of rows 64..127 is all padding
C1_CASES.append(c1case('C1-padded-live33', n=129, maps=(1, 128, 128, 2), precompute=True, live=33, period=128, save_row0=128, form='padded'))
C1_CASES.append(c1case('C1-pointmajor', n=128, maps=(1, 64, 64, 2), form='orders'))
C1_CASES.append(c1case('C1-pointmajor-init', n=128, maps=(1, 64, 64, 2), precompute=True, form='orders'))
C1_CASES.append(c1case('C1-init-rows65', n=65, precompute=True))


def geo_weights(seed, n_layers=5, skip=2):
    """Random effective weights of a stage-1 geometry network (fused.pack_geo_chains: 1 / sqrt 2 already folded in): layer 0 reads
    the 39 encoding columns, the layer in front of the skip layer has 217 outputs, the last one 257 (logit row + 256 features)."""
    g = torch.Generator().manual_seed(seed)
    Ws, bs = [], []
    for l in range(n_layers):
        fan = OCC_DPE if l == 0 else 256
        o = 257 if l == n_layers - 1 else (OCC_PE_FIRST if l == skip - 1 else 256)
        Ws.append(torch.randn(o, fan, generator=g) * (1.2 / math.sqrt(fan)))
        bs.append(torch.randn(o, generator=g) * 0.05)
    return Ws, bs


def geo_chain_model(Ws, bs, skip, pe, dtype):
    """The value chain of fused.pack_geo_chains(..., x3=True)['fwd'] in ``dtype`` on the encoding table pe [Q, 64]: every 256-row
    layer through x3dot, softplus(beta = 100), the feature head (rows 1.. of the last layer) through x3dot as well, the logit row
    (a 32-row fp32 final layer) as a plain product -> (logit [Q, 1], features [Q, 256], [softplus outputs])."""
    n = len(Ws)
    x = pe[:, :OCC_DPE].to(dtype)
    h, A = None, []
    for l in range(n - 1):
        W = Ws[l]
        if l == 0:
            z = x3dot(x, W, dtype)
        elif l == skip:
            d_a = W.shape[1] - OCC_DPE
            z = x3dot(h[:, :d_a], W[:, :d_a], dtype) + x3dot(x, W[:, d_a:], dtype)
        else:
            z = x3dot(h, W, dtype)
        h = torch.nn.functional.softplus(z + bs[l].to(dtype), beta=100)
        A.append(h)
    feat = x3dot(h, Ws[-1][1:], dtype) + bs[-1][1:].to(dtype)
    logit = h @ Ws[-1][:1].to(dtype).t() + bs[-1][:1].to(dtype)
    return logit, feat, A
