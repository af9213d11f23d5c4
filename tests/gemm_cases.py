"""Case tables and plain-torch definitions for the GEMM family (csrc/gemm.hip), path by path.

Nothing here needs a GPU: tests/test_gemm_cpu.py asserts the coverage of the tables (through the host-only plan queries
psn_gemm_plan / psn_gemm_tn_plan / psn_colsum_plan, so that no second copy of the dispatch rules lives here) and the quality of
the definitions; tests/test_gemm_gpu.py runs every case on the device.

A *case* is a plain dict.  ``build_*(case, cls)`` makes its operands (plain float32 CPU tensors, seeded per case) for one of
two operand classes:
  'int'   entries drawn from the integers in [-4, 4] ({-1, 0, 1} for the table cases near K = 2^24): every partial sum in
          every summation order is an integer below 2^24 and exact in fp32, so the kernel must EQUAL the float64 result --
          "every k row exactly once" at no tolerance.  int_bound(case) states the condition, test_gemm_cpu.py checks it.
  'real'  randn operands, for rounding quality under helpers.assert_vs_truth.
Every operand is a VIEW into a larger buffer (``place``) with guard rows in front and behind and guard columns left and
right, all of the NaN bit pattern NAN_BITS: an operand element read from outside its view poisons the result, an output
element written outside its view loses the pattern.  Output buffers start as NAN_BITS inside as well.

The definitions (``epilogue_def``, ``gemm_def``, ``splitk_def``, ``tn_item_def``, ``colsum_def``) are written out from the
comments of include/psnerf_hip.h in a chosen dtype: float64 = the truth, float32 = the reference arithmetic.
"""
import zlib

import torch

NAN_BITS = 0x7FC12345      # the pattern of tests/test_mlp_gpu.py
GR = 4                     # guard rows in front of and behind every view (a multiple of 4: the view's base keeps its alignment
                           # whatever the row stride)
RTOL = 1e-5                # linear outputs: helpers.assert_vs_truth(rtol, 'max'), the project's bound for raw kernel checks
                           # (measured worst ratio of the float32 CPU definition: 0.095 of the bound)
# nonlinear outputs: the rtol tests/test_kernels_gpu.py::test_gemm_epilogues_and_strides uses for that output, fed to
# assert_vs_truth with the float32 CPU definition as the reference arithmetic.  Measured worst ratio of that reference in
# units of the bound (test_gemm_cpu.py::test_real_reference_within_half_the_bound_gemm asserts < 0.5), over all cases:
RTOL_OUT = {
    'softplus': 1e-5,       # 0.018
    'softplus_aux': 2e-4,   # 0.004
    'sigmoid': 5e-6,        # 0.113
    'softplus_bwd': 1e-5,   # 0.009  (no earlier test: fp32 products and one sum, the linear bound)
}
INT_LIMIT = 1 << 24

EPI = dict(NONE=0, BIAS=1, BIAS_RELU=2, BIAS_SOFTPLUS=3, MUL_AUX=4, MUL_POS=5, BIAS_SIGMOID=6, ACCUM=7, MUL2=8,
           SOFTPLUS_BWD=9, MUL_AUX_RAW=10)
EPI_EXACT = ('NONE', 'BIAS', 'BIAS_RELU', 'MUL_AUX', 'MUL_POS', 'ACCUM', 'MUL2', 'MUL_AUX_RAW')   # exact on 'int' operands
NEED_BIAS = ('BIAS', 'BIAS_RELU', 'BIAS_SOFTPLUS', 'BIAS_SIGMOID')
NEED_AUX1 = ('MUL_AUX', 'MUL_POS', 'MUL2', 'SOFTPLUS_BWD', 'MUL_AUX_RAW')
NEED_AUX2 = ('MUL2', 'SOFTPLUS_BWD')
NEED_AUXOUT = ('MUL2', 'MUL_AUX_RAW')                  # BIAS_SOFTPLUS: optional
LAYOUTS = ((False, True), (False, False), (True, False), (True, True))      # (trans_a, trans_b)
BIG_M = 262017             # the smallest M with 2048 row panels of 128; the last panel has one row
ROW_BLOCK = 65536          # rows per block when a large-M case is evaluated in float64 (<= 134 MB per [block, 256] tensor)


def case_id(c):
    return c['id']


def _gen(c, cls, salt=0):
    return torch.Generator().manual_seed((zlib.crc32((c['id'] + cls).encode()) + salt) % (2 ** 31))


# --------------------------------------------------------------------------- placement: views into guarded buffers
def layout(rows, cols, mode='ok'):
    """-> (buffer rows, buffer cols, r0, c0) of a rows x cols view.
    'ok'      16-byte aligned base, ld % 4 == 0, >= 4 guard columns on both sides
    'ld'      ld % 4 == 1, base still aligned        'base'    base off by 4 bytes, ld % 4 == 0
    'rowend'  aligned, and the last 4-column group of the view ends exactly at the buffer's row end
    'w256' / 'w260'  a column slice of a 256- / 260-wide buffer starting at column 0 / 4 (cols <= 256)
    'tight'   guard rows only: the buffer is exactly as wide as the view"""
    pad = (-cols) % 4
    if mode == 'ok':
        c0, width = 4, 4 + cols + pad + 4
    elif mode == 'ld':
        c0, width = 4, 4 + cols + pad + 5
    elif mode == 'base':
        c0, width = 5, 5 + cols + pad + 3
    elif mode == 'rowend':
        c0, width = 4, 4 + cols + pad
    elif mode == 'tight':
        c0, width = 0, cols
    elif mode == 'w256':
        assert cols <= 256
        c0, width = 0, 256
    elif mode == 'w260':
        assert cols <= 256
        c0, width = 4, 260
    else:
        raise ValueError(mode)
    return rows + 2 * GR, width, GR, c0


def nan_bits(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32).view(torch.float32)


def place(t, mode='ok'):
    """The whole guarded buffer (NAN_BITS everywhere) with ``t`` copied into its view; view_of() finds the view again."""
    R, W, r0, c0 = layout(t.shape[0], t.shape[1], mode)
    whole = nan_bits(R, W)
    whole[r0:r0 + t.shape[0], c0:c0 + t.shape[1]] = t
    return whole


def view_of(whole, rows, cols, mode='ok'):
    R, W, r0, c0 = layout(rows, cols, mode)
    assert tuple(whole.shape) == (R, W)
    return whole[r0:r0 + rows, c0:c0 + cols]


def guards_intact(whole, rows, cols, mode='ok'):
    """Everything outside the view still has the bits of NAN_BITS (works on any device)."""
    R, W, r0, c0 = layout(rows, cols, mode)
    bits = whole.view(torch.int32).clone()
    bits[r0:r0 + rows, c0:c0 + cols] = NAN_BITS
    return bool((bits == NAN_BITS).all())


def untouched(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def place_vec(v):
    """1-D operand (bias, column sums) inside 8 guard floats on each side: (whole, slice)."""
    whole = nan_bits(v.numel() + 16)
    whole[8:8 + v.numel()] = v
    return whole


def vec_of(whole, n):
    return whole[8:8 + n]


def vec_guards_intact(whole, n):
    return untouched(whole[:8]) and untouched(whole[8 + n:])


def draw(g, shape, cls, lo=-4, hi=4):
    if cls == 'int':
        return torch.randint(lo, hi + 1, shape, generator=g).float()
    return torch.randn(shape, generator=g)


# --------------------------------------------------------------------------- definitions
def epilogue_def(acc, epi, bias=None, aux1=None, aux2=None, c_in=None, want_aux=True, fault=None):
    """(C, aux_out or None) of include/psnerf_hip.h's PSN_EPI_* in the dtype of ``acc``.  ``fault`` seeds a wrong formulation
    (test_gemm_cpu.py): 'bias_shift' = the bias of column n applied to n + 1, 'pos_ge' = MUL_POS with >=."""
    if bias is not None and fault == 'bias_shift':
        bias = torch.roll(bias, 1)
    z = acc + bias if epi in NEED_BIAS else acc
    if epi == 'NONE':
        return acc, None
    if epi == 'BIAS':
        return z, None
    if epi == 'BIAS_RELU':
        return z.clamp(min=0), None
    if epi == 'BIAS_SOFTPLUS':
        return torch.nn.functional.softplus(z, beta=100, threshold=20), (torch.sigmoid(100 * z) if want_aux else None)
    if epi == 'MUL_AUX':
        return acc * aux1, None
    if epi == 'MUL_POS':
        return acc * ((aux1 >= 0) if fault == 'pos_ge' else (aux1 > 0)).to(acc.dtype), None
    if epi == 'BIAS_SIGMOID':
        return torch.sigmoid(z), None
    if epi == 'ACCUM':
        return c_in + acc, None
    if epi == 'MUL2':
        return acc * aux1, acc * aux2
    if epi == 'SOFTPLUS_BWD':
        return aux1 * (acc + 100 * aux2 * (1 - aux1)), None
    if epi == 'MUL_AUX_RAW':
        return acc * aux1, acc
    raise ValueError(epi)


def outputs_of(epi, want_aux=True):
    """The names of the tolerance class of (C, aux_out) under RTOL_OUT, None = linear."""
    return {'BIAS_SOFTPLUS': ('softplus', 'softplus_aux' if want_aux else None), 'BIAS_SIGMOID': ('sigmoid', None),
            'SOFTPLUS_BWD': ('softplus_bwd', None)}.get(epi, (None, None))


def gemm_def(op, dtype, rows=None, fault=None):
    """The definition of one psn_gemm call on the operands ``op`` (build_gemm) in ``dtype``: (C, aux_out or None, colsum_a or
    None); ``rows`` = a slice of the M rows (large-M cases are evaluated block by block)."""
    c = op['case']
    ta, tb = c['ta'], c['tb']
    rows = slice(None) if rows is None else rows
    A = op['A'].to(dtype)
    A = A[:, rows].t() if ta else A[rows]
    B = op['B'].to(dtype)
    B = B.t() if tb else B
    if fault == 'col_shift':          # a column group shifted by four
        B = torch.roll(B, 4, dims=1)
    cut = lambda t: None if t is None else t[rows].to(dtype)
    acc = splitk_def(A, B, c.get('k_chunk') or A.shape[1], fault=fault)
    C, aux = epilogue_def(acc, c['epi'], None if op['bias'] is None else op['bias'].to(dtype), cut(op['aux1']), cut(op['aux2']),
                          cut(op['c_in']), want_aux=c.get('aux_out', True), fault=fault)
    cs = A.sum(1) if c.get('colsum') else None
    return C, aux, cs


def splitk_def(A, B, kc, fault=None):
    """sum over the K slices of ``kc`` rows of A[:, slice] @ B[slice] (A [M, K], B [K, N]): the split-K sum in the order of the
    reduction kernel.  Seeded faults: 'drop_seam' = the first row of the second slice (or the last row, with one slice) is
    lost, 'dup_last' = the last row counted twice (the prefetch clamp without its mask)."""
    K = A.shape[1]
    acc = None
    for k0 in range(0, K, kc):
        part = A[:, k0:k0 + kc] @ B[k0:k0 + kc]
        acc = part if acc is None else acc + part
    if fault == 'drop_seam':
        k = kc if kc < K else K - 1
        acc = acc - A[:, k:k + 1] @ B[k:k + 1]
    if fault == 'dup_last':
        acc = acc + A[:, K - 1:K] @ B[K - 1:K]
    return acc


def table_rows(K, div, mod, fault=None):
    """Row of the table that row k of the product reads: (k // div) % mod.  Seeded fault 'div_off': the quotient is one short
    at the multiples of div (a reciprocal estimate left uncorrected)."""
    k = torch.arange(K, dtype=torch.int64)
    q = torch.div(k, div, rounding_mode='floor')
    if fault == 'div_off':
        q = q - ((k % div == 0) & (k > 0)).long()
    return q % mod


def tn_item_def(it, K, dtype, fault=None, kc=None):
    """One item of psn_gemm_tn_grouped on CPU operands (dict as for hip.gemm_tn_grouped, plus 'base' = the prior content of
    an accumulated result): (C, colsum or None) in ``dtype``."""
    kr = it['A'].shape[0]
    if it.get('b_div') or it.get('b_mod'):
        # C = S^T T with S[r] = the sum of the rows of A that read table row r (index_add_, in blocks of rows: K may be 2^24)
        def through_table(T, div, mod):
            idx = table_rows(K, div, mod, fault)
            S = torch.zeros(T.shape[0], it['A'].shape[1], dtype=dtype)
            for k0 in range(0, K, 1 << 22):
                S.index_add_(0, idx[k0:k0 + (1 << 22)], it['A'][k0:k0 + (1 << 22)].to(dtype))
            return S.t() @ T.to(dtype)
        C = through_table(it['B'], max(int(it.get('b_div', 0)), 1), int(it.get('b_mod') or it['B'].shape[0]))
        if it.get('B_tab2') is not None:
            C = torch.cat([C, through_table(it['B_tab2'], int(it['b2_div']), int(it.get('b2_mod', it['B_tab2'].shape[0])))], 1)
    else:
        C = splitk_def(it['A'].to(dtype).t(), it['B'].to(dtype), kc or kr, fault=fault)
    if it.get('A2') is not None:
        C = C + it['A2'].to(dtype).t() @ it['B2'].to(dtype)
    if it.get('accumulate'):
        C = it['base'].to(dtype) + C
    return C, (it['A'].to(dtype).sum(0) if it.get('colsum') else None)


def colsum_def(X, w, base, dtype, block=1024):
    """out[n] = sum_m X[m, n], or out[j, n] = sum_m w[m, j] X[m, n]; + base under accumulate.  Summed in blocks of 1024 rows
    and then over the blocks, as every careful evaluation would: one running float32 sum over 262,145 rows drifts by up to
    0.9 of the bound, depending on the host's BLAS, and could not serve as the reference arithmetic."""
    X = X.to(dtype).contiguous()
    M, N = X.shape
    nb = M // block
    w = None if w is None else w.to(dtype).contiguous()

    def part(x, ww):      # [b, rows, N] (, [b, rows, n_w]) -> [b, N] or [b, n_w, N]
        return x.sum(1) if ww is None else torch.bmm(ww.transpose(1, 2), x)
    main = part(X[:nb * block].view(nb, block, N), None if w is None else w[:nb * block].view(nb, block, w.shape[1])).sum(0)
    out = main + part(X[None, nb * block:], None if w is None else w[None, nb * block:])[0]
    return out if base is None else base.to(dtype) + out


# --------------------------------------------------------------------------- psn_gemm cases (families A - D)
def gemm_case(fam, name, ta, tb, M, N, K, epi='NONE', split_k=1, colsum=False, modes=None, aux_out=True, k_chunk=None,
               classes=None):
    modes = dict(dict(A='ok', B='ok', C='ok', aux1='ok', aux2='ok', aux_out='ok'), **(modes or {}))
    if classes is None:
        classes = ('int', 'real') if epi in EPI_EXACT else ('real',)
    mtag = ''.join('-%s_%s' % kv for kv in sorted(modes.items()) if kv[1] != 'ok')
    cid = '%s-%s-%s%s-%dx%dx%d-%s%s%s%s' % (fam, name, 'T' if ta else 'N', 'T' if tb else 'N', M, N, K, epi,
                                            '-s%d' % split_k if split_k > 1 else '', '-cs' if colsum else '', mtag)
    return dict(id=cid, family=fam, ta=ta, tb=tb, M=M, N=N, K=K, epi=epi, split_k=split_k, colsum=colsum, modes=modes,
                aux_out=aux_out, k_chunk=k_chunk, classes=classes)


def build_gemm(c, cls):
    """Operands of a psn_gemm case: the logical matrices (CPU float32) and the guarded buffers that hold them."""
    g = _gen(c, cls)
    M, N, K, epi = c['M'], c['N'], c['K'], c['epi']
    A = draw(g, (K, M) if c['ta'] else (M, K), cls)
    B = draw(g, (N, K) if c['tb'] else (K, N), cls)
    soft = epi in ('BIAS_SOFTPLUS',) and cls == 'real'
    if soft:
        B = B * 0.02       # pre-activations z * 0.02 as in test_gemm_epilogues_and_strides: sigmoid(100 z) is not saturated
    bias = aux1 = aux2 = c_in = None
    if epi in NEED_BIAS:
        bias = draw(g, (N,), cls) * (0.02 if soft else 1.0)
    if epi in NEED_AUX1:
        aux1 = torch.sigmoid(torch.randn(M, N, generator=g)) if epi == 'SOFTPLUS_BWD' else draw(g, (M, N), cls)
        if epi == 'MUL_POS':     # zeros among the signs, in both classes: > 0 and >= 0 differ there
            aux1 = aux1 * (torch.rand(M, N, generator=g) > 0.25).float()
    if epi in NEED_AUX2:
        aux2 = draw(g, (M, N), cls)
    if epi == 'ACCUM':
        c_in = draw(g, (M, N), cls)
    return dict(case=c, cls=cls, A=A, B=B, bias=bias, aux1=aux1, aux2=aux2, c_in=c_in)


def gemm_buffers(op, to=lambda t: t):
    """The guarded buffers of a built case, moved with ``to``, and the views the call takes: dict name -> (whole, view)."""
    c = op['case']
    m = c['modes']
    M, N = c['M'], c['N']
    res = {}
    for name, t, mode in (('A', op['A'], m['A']), ('B', op['B'], m['B']), ('aux1', op['aux1'], m['aux1']),
                          ('aux2', op['aux2'], m['aux2'])):
        if t is not None:
            whole = to(place(t, mode))
            res[name] = (whole, view_of(whole, t.shape[0], t.shape[1], mode))
    whole = to(nan_bits(*layout(M, N, m['C'])[:2]) if op['c_in'] is None else place(op['c_in'], m['C']))
    res['C'] = (whole, view_of(whole, M, N, m['C']))
    has_aux_out = c['epi'] in NEED_AUXOUT or (c['epi'] == 'BIAS_SOFTPLUS' and c['aux_out'])
    if has_aux_out:
        whole = to(nan_bits(*layout(M, N, m['aux_out'])[:2]))
        res['aux_out'] = (whole, view_of(whole, M, N, m['aux_out']))
    if op['bias'] is not None:
        whole = to(place_vec(op['bias']))
        res['bias'] = (whole, vec_of(whole, N))
    if c['colsum']:
        whole = to(nan_bits(M + 16))
        res['colsum'] = (whole, vec_of(whole, M))
    return res


def gemm_plan_of(c, ws_addr=0):
    """psn_gemm_plan for the placement of this case (CPU buffers: torch aligns them to 64 bytes, the device to more)."""
    from psnerf_amd import hip
    M, N, K, m = c['M'], c['N'], c['K'], c['modes']
    shp = dict(A=(K, M) if c['ta'] else (M, K), B=(N, K) if c['tb'] else (K, N))
    v = lambda name, r, k: view_of(torch.empty(layout(r, k, m[name])[:2]), r, k, m[name])
    e = c['epi']
    return hip.gemm_plan(v('A', *shp['A']), v('B', *shp['B']), v('C', M, N), c['ta'], c['tb'],
                         aux_in=v('aux1', M, N) if e in NEED_AUX1 else None, aux_in2=v('aux2', M, N) if e in NEED_AUX2 else None,
                         aux_out=v('aux_out', M, N) if (e in NEED_AUXOUT or (e == 'BIAS_SOFTPLUS' and c['aux_out'])) else None,
                         split_k=c['split_k'], workspace_addr=ws_addr)


def gemm_int_bound(c):
    """Largest magnitude any partial sum or epilogue value of an 'int' case can reach: K products of at most 16, then one
    factor of at most 4 or one addend of at most 4."""
    return c['K'] * 16 * (4 if c['epi'] in ('MUL_AUX', 'MUL2', 'MUL_AUX_RAW') else 1) + 4


A_M, A_N, A_K = (1, 127, 128, 129, 257), (1, 3, 127, 128, 130, 217, 289), (1, 15, 16, 17, 33, 126)


def _family_a():
    """128-column tiles: a pairwise-covering subset of M x N x K (test_gemm_cpu.py checks that it covers every pair) in all four
    layouts, and the a_vec / b_vec fallbacks on each side."""
    cases = []
    shapes = [(A_M[(i + i // 7) % 5], A_N[i % 7], A_K[i // 7]) for i in range(42)]
    for i, (M, N, K) in enumerate(shapes):
        for ta, tb in LAYOUTS:
            cases.append(gemm_case('A', 'pair', ta, tb, M, N, K))
    for i, (M, N, K) in enumerate([(129, 130, 33), (257, 217, 17), (128, 3, 126), (127, 289, 16)]):
        for ta, tb in LAYOUTS:
            for side in ('A', 'B'):
                for mode in ('ld', 'base'):
                    cases.append(gemm_case('A', 'mis', ta, tb, M, N, K, modes={side: mode}))
    return cases


def _family_b():
    """256-column tiles: by M (2048 row panels) in all four layouts, and through split-K at small M."""
    cases = []
    for ta, tb in LAYOUTS:
        for N in (132, 256):
            for K in (16, 33):
                cases.append(gemm_case('B', 'rows', ta, tb, BIG_M, N, K))
    for M in (130, 256):
        for N in (256, 255):
            for epi in ('NONE', 'ACCUM'):
                cases.append(gemm_case('B', 'split', True, False, M, N, 16384, epi=epi, split_k=1024, colsum=True, k_chunk=16))
    return cases


MIS_STATES = [{}] + [{name: mode} for name in ('C', 'aux1', 'aux2', 'aux_out') for mode in ('ld', 'base')]


def _family_c():
    """Every epilogue x {trans_b, one other layout} x NT x N in {256 all-full4, 217 ragged last float4, 3 no full4} x alignment
    state.  NT = 2 at M = 257: the full cross with the alignment states that the epilogue has operands for.  NT = 4 at M =
    BIG_M (N = 3 has no 256-column tile): each epilogue at N = 256 aligned in trans_b, and at N = 217 in the other layout with
    one misaligned operand, rotating through the states."""
    cases = []
    rot = 0
    for e in EPI:
        has = dict(C=True, aux1=e in NEED_AUX1, aux2=e in NEED_AUX2, aux_out=e in NEED_AUXOUT or e == 'BIAS_SOFTPLUS')
        states = [s for s in MIS_STATES if all(has[k] for k in s)]
        for (ta, tb) in ((False, True), (False, False)):
            for N in (256, 217, 3):
                for s in states:
                    if tb is False and s and N == 256:
                        continue        # the second layout runs the misaligned states at the two ragged widths only
                    cases.append(gemm_case('C', 'nt2', ta, tb, 257, N, 33, epi=e, modes=s))
        cases.append(gemm_case('C', 'nt4', False, True, BIG_M, 256, 16, epi=e))
        mis = [s for s in states if s]
        cases.append(gemm_case('C', 'nt4', True, False, BIG_M, 217, 17, epi=e, modes=mis[rot % len(mis)]))
        rot += 1
    cases.append(gemm_case('C', 'noaux', False, True, 257, 217, 33, epi='BIAS_SOFTPLUS', aux_out=False))
    cases.append(gemm_case('C', 'noaux', False, True, 257, 256, 33, epi='BIAS_SOFTPLUS', aux_out=False))
    return cases


def _family_d():
    """Split-K seams of psn_gemm, trans_a, M = 256: the last slice has 1, 15 and 16 rows; the library's slice count is below the
    requested one (K = 100, 5 requested, 32-row chunks -> 4); the request collapses to one slice (K = 5, 16 requested) and
    EPI_ACCUM and the column sums go straight to the caller's buffers."""
    cases = []
    for N in (382, 217):
        for K, s, kc in ((33, 2, 32), (47, 2, 32), (48, 2, 32), (100, 5, 32)):
            for epi in ('NONE', 'ACCUM'):
                cases.append(gemm_case('D', 'seam', True, False, 256, N, K, epi=epi, split_k=s, colsum=True, k_chunk=kc))
        cases.append(gemm_case('D', 'collapse', True, False, 256, N, 5, epi='ACCUM', split_k=16, colsum=True, k_chunk=16))
    return cases


GEMM_CASES = _family_a() + _family_b() + _family_c() + _family_d()

# argument checks of psn_gemm: (name, epilogue, what is withheld or added) -> RuntimeError, nothing written
ARG_CHECKS = [('no-aux_in', 'MUL_AUX', 'aux1'), ('no-aux_in-pos', 'MUL_POS', 'aux1'), ('no-aux_in2', 'MUL2', 'aux2'),
              ('no-aux_in2-bwd', 'SOFTPLUS_BWD', 'aux2'), ('no-aux_out', 'MUL2', 'aux_out'), ('no-aux_out-raw', 'MUL_AUX_RAW', 'aux_out'),
              ('no-bias', 'BIAS', 'bias'), ('no-bias-relu', 'BIAS_RELU', 'bias'), ('no-bias-softplus', 'BIAS_SOFTPLUS', 'bias'),
              ('no-bias-sigmoid', 'BIAS_SIGMOID', 'bias')] + \
             [('split-' + e, e, 'split') for e in EPI if e not in ('NONE', 'ACCUM')] + [('colsum-without-trans_a', 'NONE', 'colsum')]


# --------------------------------------------------------------------------- psn_gemm_tn_grouped cases (families E - G)
TN_K = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 193)
TN_K_SLICES = (513, 4099)
E_SHAPES = ((256, 256), (217, 256), (129, 256), (256, 200), (130, 129))
F_SHAPES = ((256, 39), (256, 64), (130, 33), (129, 1), (256, 4))


def _tn_case(fam, name, K, items, split_k=1, x3=True, classes=('int', 'real'), lo=-4, hi=4):
    return dict(id='%s-%s-K%d' % (fam, name, K), family=fam, K=K, items=items, split_k=split_k, x3=x3, classes=classes,
                lo=lo, hi=hi)


def _it(M, N, rows=None, A='ok', B='ok', C='ok', two=None, colsum=False, accumulate=False, **table):
    """Item spec: M, N, rows (None = K; fewer = a k_rows prefix), placement modes, two = (A2 mode, B2 mode), table keys
    b_div / b_mod / tab_rows (rows of the table B) / tab2 = (columns, rows, b2_div, b2_mod)."""
    return dict(M=M, N=N, rows=rows, A=A, B=B, C=C, two=two, colsum=colsum, accumulate=accumulate, **table)


def _trio(M, N, K, bmode):
    """The three items every E / F shape runs in one group: a single product with column sums whose A is a slice of a 260-wide
    and whose B of a 256-wide buffer (F: B ends at its buffer's row end); two products with column sums, the second pair in
    256- / 260-wide buffers; a k_rows prefix that ends inside a k-tile (K - 1 rows where K is a multiple of 32: a 31-row last
    tile for every loop regime; K - 5 elsewhere), accumulated."""
    items = [_it(M, N, A='w260', B=bmode[0], colsum=True),
             _it(M, N, B=bmode[1], two=('w256', bmode[2]), colsum=True)]
    if K > 1:
        items.append(_it(M, N, rows=K - 1 if (K % 32 == 0 or K <= 5) else K - 5, B=bmode[1], accumulate=True, colsum=True))
    return items


def _family_e():
    cases = []
    for (M, N) in E_SHAPES:
        for K in TN_K + TN_K_SLICES:
            cases.append(_tn_case('E', '%dx%d' % (M, N), K, _trio(M, N, K, ('w256', 'ok', 'w260'))))
    return cases


def _family_f():
    cases = []
    for (M, N) in F_SHAPES:
        for K in TN_K + TN_K_SLICES:
            cases.append(_tn_case('F', '%dx%d' % (M, N), K, _trio(M, N, K, ('rowend', 'rowend', 'rowend')), x3=False))
    return cases


FASTDIV_K = (INT_LIMIT - 16, INT_LIMIT, INT_LIMIT + 16)
FASTDIV_ZERO_ROWS = (32, 64)      # rows [32, 64) of A are zero in the fastdiv cases: at most K - 32 <= 2^24 nonzero terms


def _mixed_items(n):
    """n items that mix the three kinds, tables and accumulation (groups of 13 and 25 = 2 and 3 launches)."""
    kinds = [lambda: _it(256, 256, colsum=True), lambda: _it(256, 39, B='rowend', colsum=True), lambda: _it(100, 70),
             lambda: _it(130, 129, accumulate=True), lambda: _it(64, 8, b_div=3, b_mod=5, tab_rows=5, colsum=True),
             lambda: _it(217, 256, A='ld'), lambda: _it(1, 1, accumulate=True, colsum=True)]
    return [kinds[i % len(kinds)]() for i in range(n)]


def _family_g():
    cases = []
    # the 128 x 128 tiles: M <= 128, ragged and multi-tile N, strided and misaligned operands, two products, a prefix
    for K in (1, 15, 16, 17, 33, 100):
        cases.append(_tn_case('G', 'tile', K, [
            _it(128, 128, colsum=True), _it(1, 1, colsum=True), _it(127, 130, A='ld', colsum=True), _it(3, 289, B='base'),
            _it(100, 217, two=('ok', 'ld'), colsum=True, accumulate=True), _it(128, 3, C='ld', accumulate=True)]
            + ([_it(65, 64, rows=K - 1, colsum=True)] if K > 1 else []), split_k=1, x3=False))
    for K, s in ((100, 3), (513, 4), (4099, 16)):
        cases.append(_tn_case('G', 'tile-split', K, [
            _it(128, 128, colsum=True), _it(127, 130, A='base', colsum=True), _it(100, 217, two=('ok', 'ok'), colsum=True),
            _it(65, 64, rows=K - 7, colsum=True, accumulate=True)], split_k=s, x3=False))
    # items that would be 256 x 256 or tall tiles but for one misaligned operand: back to the 128 x 128 tiles
    for K in (33, 193, 513):
        cases.append(_tn_case('G', 'fallback', K, [
            _it(256, 256, A='ld', colsum=True), _it(256, 256, B='base', colsum=True), _it(217, 256, two=('base', 'ok'), colsum=True),
            _it(256, 200, two=('ok', 'ld')), _it(256, 39, A='base', colsum=True), _it(256, 64, B='ld', colsum=True),
            _it(130, 33, two=('ld', 'ok'), colsum=True), _it(256, 256, colsum=True), _it(256, 39, B='rowend', colsum=True)],
            split_k=2 if K > 100 else 1))
    # tables: one table, a modulo that wraps and one that cannot, two tables side by side, in the aligned and the scalar form
    Ns, V = 37, 5
    cases.append(_tn_case('G', 'table', Ns * V, [
        _it(256, 64, b_div=1, b_mod=Ns, tab_rows=Ns, colsum=True), _it(256, 64, b_div=Ns, b_mod=V, tab_rows=V),
        _it(100, 39, b_div=Ns, b_mod=3, tab_rows=3, colsum=True), _it(256, 64, b_div=7, b_mod=Ns, tab_rows=Ns, B='ld'),
        _it(256, 128, b_div=1, b_mod=Ns, tab_rows=Ns, tab2=(64, V, Ns, V), colsum=True),
        _it(130, 75, b_div=2, b_mod=Ns, tab_rows=Ns, tab2=(39, V, Ns, 2), accumulate=True),
        _it(256, 256, colsum=True)], split_k=2))
    cases.append(_tn_case('G', 'group13', 193, _mixed_items(13), split_k=2))
    cases.append(_tn_case('G', 'group25', 97, _mixed_items(25), split_k=1))
    # fastdiv24 at both sides of 2^24: A [K, 1] of {-1, 0, 1} (M = 1 keeps the case at a few seconds) shared by 12 table items
    for K in FASTDIV_K:
        items = []
        for d in (1, 2, 3, 7, 777, 4096):
            q = (K - 1) // d + 1            # distinct quotients
            items.append(_it(1, 8, b_div=d, b_mod=5, tab_rows=5))                                 # the modulo wraps
            items.append(_it(1, 8, b_div=d, b_mod=min(q, 65536) if d >= 3 else 7, tab_rows=min(q, 65536) if d >= 3 else 7))
        cases.append(_tn_case('G', 'fastdiv', K, items, split_k=256, x3=False, classes=('int',), lo=-1, hi=1))
    return cases


TN_CASES = _family_e() + _family_f() + _family_g()


def build_tn(c, cls):
    """CPU operands of a grouped case: a list of item dicts in the form of hip.gemm_tn_grouped, each with its guarded buffers
    under 'whole' (name -> buffer) and its 'spec'.  The fastdiv cases share one A among their items.  cls = None: buffers of
    the right shape and placement without content (for the plan queries)."""
    g = _gen(c, cls or '')
    K = c['K']
    shared = {}
    items = []
    for s in c['items']:
        rows = K if s['rows'] is None else s['rows']
        M, N = s['M'], s['N']
        it = dict(spec=s, whole={}, colsum=s['colsum'], accumulate=s['accumulate'])

        def put(name, shape, mode, it=it):
            if cls is None:
                it['whole'][name] = torch.empty(layout(shape[0], shape[1], mode)[:2])
            else:
                t = draw(g, shape, cls, c['lo'], c['hi'])
                if 'fastdiv' in c['id'] and name == 'A':
                    t[FASTDIV_ZERO_ROWS[0]:FASTDIV_ZERO_ROWS[1]] = 0
                it['whole'][name] = place(t, mode)
            it[name] = view_of(it['whole'][name], shape[0], shape[1], mode)
        if 'fastdiv' in c['id']:
            if not shared:
                put('A', (K, M), 'tight')
                shared.update(whole=it['whole']['A'], A=it['A'])
            it['whole']['A'], it['A'] = shared['whole'], shared['A']
        else:
            put('A', (rows, M), s['A'])
        if s.get('b_div'):
            n1 = N - (s['tab2'][0] if s.get('tab2') else 0)
            put('B', (s['tab_rows'], n1), s['B'])
            it['b_div'], it['b_mod'] = s['b_div'], s['b_mod']
            if s.get('tab2'):
                cols, trows, d2, m2 = s['tab2']
                put('B_tab2', (trows, cols), s['B'])
                it['b2_div'], it['b2_mod'] = d2, m2
        else:
            put('B', (rows, N), s['B'])
        if s['two']:
            put('A2', (rows, M), s['two'][0])
            put('B2', (rows, N), s['two'][1])
        put('out', (M, N), s['C'])
        if s['accumulate'] and cls is not None:
            it['base'] = it['out'].clone()
        elif cls is not None:
            it['whole']['out'].view(torch.int32).fill_(NAN_BITS)
        items.append(it)
    return items


def a_mode(c, s):
    return 'tight' if 'fastdiv' in c['id'] else s['A']


TN_OPERANDS = ('A', 'B', 'A2', 'B2', 'B_tab2', 'out')


def tn_to(c, items, to):
    """The items of build_tn with their buffers moved by ``to`` (a buffer shared by several items moves once)."""
    moved = {}
    res = []
    for it in items:
        s = it['spec']
        new = {k: v for k, v in it.items() if k not in TN_OPERANDS + ('whole', 'base')}
        new['whole'] = {}
        for name in TN_OPERANDS:
            if name in it['whole']:
                w = it['whole'][name]
                if id(w) not in moved:
                    moved[id(w)] = to(w)
                new['whole'][name] = moved[id(w)]
                mode = {'A': a_mode(c, s), 'B': s['B'], 'B_tab2': s['B'], 'out': s['C']}.get(name) or s['two'][0 if name == 'A2' else 1]
                v = it[name]
                new[name] = view_of(new['whole'][name], v.shape[0], v.shape[1], mode)
        res.append(new)
    return res


def tn_chunks(items):
    return [items[i:i + 12] for i in range(0, len(items), 12)]


def tn_int_bound(c):
    """'int' exactness: K * 16 (two products: twice that) + 4 for an accumulated base; the {-1, 0, 1} cases: the nonzero rows
    of A."""
    if c['hi'] == 1:
        return c['K'] - (FASTDIV_ZERO_ROWS[1] - FASTDIV_ZERO_ROWS[0])
    return c['K'] * 16 * 2 + 4


# --------------------------------------------------------------------------- psn_colsum cases (family H)
H_N, H_M = (1, 39, 256, 260, 289, 512), (0, 1, 3, 127, 129, 70001)
H_NW = (0, 1, 3, 4)


def _family_h():
    """N x M crossed in full with n_w, the placement of X and accumulate rotating (test_gemm_cpu.py: every n_w meets both
    partial kernels); M = 262,145 (nblocks at its cap of 2048) once per kernel and per n_w class."""
    cases = []
    i = 0
    for N in H_N:
        for M in H_M:
            # N = 256 is the one width both partial kernels can take: every n_w there, under every placement across the M
            for j, n_w in enumerate(H_NW if N == 256 else (H_NW[i % 4], H_NW[(i + 2) % 4])):
                mode = ('ok', 'w260' if N <= 256 else 'ok', 'ld', 'base')[(i + j) % 4]
                acc = (i + j) % 3 == 0
                cases.append(dict(id='H-%dx%d-w%d-%s%s' % (M, N, n_w, mode, '-acc' if acc else ''), family='H', M=M, N=N,
                                  n_w=n_w, mode=mode, accumulate=acc, classes=('int', 'real')))
            i += 1
    for N, n_w, mode in ((256, 0, 'ok'), (256, 4, 'ok'), (39, 3, 'ok'), (1, 1, 'ok'), (256, 1, 'ld')):
        cases.append(dict(id='H-262145x%d-w%d-%s' % (N, n_w, mode), family='H', M=262145, N=N, n_w=n_w, mode=mode,
                          accumulate=n_w == 3, classes=('int', 'real')))
    return cases


COLSUM_CASES = _family_h()


def build_colsum(c, cls):
    g = _gen(c, cls)
    X = draw(g, (c['M'], c['N']), cls)
    w = draw(g, (c['M'], c['n_w']), cls) if c['n_w'] else None
    shape = (c['n_w'], c['N']) if c['n_w'] else (c['N'],)
    base = draw(g, shape, cls) if c['accumulate'] else None
    return dict(case=c, X=X, w=w, base=base, shape=shape)


def colsum_int_bound(c):
    return c['M'] * 16 + 4


ALL_CASES = GEMM_CASES + TN_CASES + COLSUM_CASES
assert len(set(c['id'] for c in ALL_CASES)) == len(ALL_CASES), 'case ids must be unique'


# --------------------------------------------------------------------------- the checks both test modules apply
def row_blocks(M):
    return [slice(r, min(M, r + ROW_BLOCK)) for r in range(0, max(M, 1), ROW_BLOCK)]


def check_int(name, got, truth):
    """'int' class: the kernel's float32 values EQUAL the float64 (or int64) result."""
    got, want = got.detach().cpu(), truth.to(torch.float32)
    assert got.shape == want.shape, '%s: shape %s vs %s' % (name, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = ~(got == want)
        first = bad.reshape(-1).nonzero()[0].item()
        raise AssertionError('%s: %d of %d elements differ from the exact result, first at flat index %d: %r vs %r'
                             % (name, int(bad.sum()), bad.numel(), first, got.reshape(-1)[first].item(), want.reshape(-1)[first].item()))


def check_real(name, got, ref, truth, rtol, atol='max'):
    """'real' class: helpers.assert_vs_truth with the float32 CPU definition ``ref`` as the reference arithmetic.
    -> (worst r_hip, worst r_ref)."""
    from tests.helpers import assert_vs_truth
    return assert_vs_truth(name, got.detach().cpu().numpy(), ref.numpy(), truth.numpy(), rtol, atol)


def gemm_outputs(c):
    """[(name, index into gemm_def's result, rtol)] of the outputs a psn_gemm case has."""
    kc, ka = outputs_of(c['epi'], c['aux_out'])
    res = [('C', 0, RTOL_OUT.get(kc, RTOL))]
    if c['epi'] in NEED_AUXOUT or (c['epi'] == 'BIAS_SOFTPLUS' and c['aux_out']):
        res.append(('aux_out', 1, RTOL_OUT.get(ka, RTOL)))
    if c['colsum']:
        res.append(('colsum', 2, RTOL))
    return res
