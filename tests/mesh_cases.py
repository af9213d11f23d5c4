"""Edge cases for the mesh-extraction kernels (csrc/mesh.hip) and their numpy definition (psnerf_amd/stage1/extracting.py), shared
by tests/test_mesh_cpu.py, tests/test_mesh_gpu.py and tools/gen_golden_mesh.py.  Plain numpy, no GPU.

Fields on the (R + 1)^3 lattice (float32, seeded by name and R), thresholds as the double the kernels receive, the
(resolution0, depth) pairs of the refinement, the grids of the marching-cubes tests, and a lock-step driver that runs a HostMISE
one round at a time and records every intermediate state a device round can be compared with.

Tie semantics the cases exist for: a known value == threshold is both ">= thr" and "<= thr", so ONE such point makes every leaf
voxel whose closed cube contains it active; in marching cubes value <= thr is inside, and a crossing next to a tie lies exactly
on a lattice point.  A known NaN is neither, +-1e-40 against thr = 0 are no ties (nothing may flush them to zero), -0.0 is one."""
import hashlib
import zlib

import numpy as np

from tests import mesh_fields as mf

THR_ZERO = 0.0
THR_LOGIT_03 = float(np.log(0.3) - np.log(1. - 0.3))   # extracting.iso_value(0.3) = -0.847...: no float32 value equals it
THR_TIE = float(np.float32(-0.375))                    # a float32 value: grid values can equal it exactly
assert float(np.float32(THR_LOGIT_03)) != THR_LOGIT_03 and float(np.float32(THR_TIE)) == THR_TIE

# (resolution0, depth): depth 1 (no child level at all), resolution0 1 (one-thread levels), odd and non-power-of-two resolutions
# 6, 12, 20, 24, 48 (the float32 point formula divides by them), at most 49^3 grid points
MISE_PAIRS = [(1, 1), (1, 4), (2, 3), (3, 2), (5, 2), (6, 1), (3, 4)]
BOX_SIZES = [2.4, 2.0]
MC_SIZES = [2, 7, 12, 15]                              # points per axis: 1, 2, 9 and 16 runs of 256 cells ((n + 1)^3 = 4096 for 15)


def _rng(name, R):
    return np.random.RandomState(zlib.crc32(('%s/%d' % (name, R)).encode()) & 0x7fffffff)


def ternary(R):
    """Values drawn from {-1, 0, +1}: ties against thr = 0 everywhere."""
    return _rng('ternary', R).randint(-1, 2, size=(R + 1,) * 3).astype(np.float32)


def sparse_tie(R, t):
    """All +1 except about 2 % of the points, and the lattice origin, set to exactly t: at thr = t every bit of activity comes
    from a tie (the origin is a base point of every (resolution0, depth), so there always is some)."""
    f = np.ones((R + 1,) * 3, dtype=np.float32)
    f[_rng('sparse_tie', R).rand(R + 1, R + 1, R + 1) < 0.02] = np.float32(t)
    f[0, 0, 0] = np.float32(t)
    return f


def tie_checker(R):
    """mesh_fields.checker with every 7th value (x-major) set to -0.375."""
    f = mf.checker(R, seed=R).copy()
    f.reshape(-1)[::7] = np.float32(-0.375)
    return f


def nonfinite(R):
    """mesh_fields.checker with about 10 % +inf, 10 % -inf, 5 % NaN, 5 % 1e-40, 5 % -1e-40 (float32 denormals) and 3 % -0.0."""
    f = mf.checker(R, seed=R).copy()
    u = _rng('nonfinite', R).rand(R + 1, R + 1, R + 1)
    for lo, hi, val in ((0.00, 0.10, np.inf), (0.10, 0.20, -np.inf), (0.20, 0.25, np.nan), (0.25, 0.30, 1e-40), (0.30, 0.35, -1e-40),
                        (0.35, 0.38, -0.0)):
        f[(u >= lo) & (u < hi)] = np.float32(val)
    return f


FIELDS = {
    'checker': lambda R: mf.checker(R, seed=R),
    'sphere_rod_torus': mf.sphere_rod_torus,
    'ternary': ternary,
    'sparse_tie0': lambda R: sparse_tie(R, 0.0),
    'sparse_tie375': lambda R: sparse_tie(R, -0.375),
    'tie_checker': tie_checker,
    'nonfinite': nonfinite,
    'all_tie375': lambda R: np.full((R + 1,) * 3, -0.375, dtype=np.float32),
    'all_above': lambda R: np.ones((R + 1,) * 3, dtype=np.float32),
}
THRESHOLDS = {'zero': THR_ZERO, 'logit03': THR_LOGIT_03, 'tie375': THR_TIE}
REFINING = ('checker', 'ternary')                      # the fields resolution0 = 1 is paired with: elsewhere nothing happens there
_cache = {}


def field(name, R):
    """The field ``name`` on the (R + 1)^3 lattice (computed once; read-only)."""
    if (name, R) not in _cache:
        f = np.ascontiguousarray(FIELDS[name](R), dtype=np.float32)
        f.setflags(write=False)
        _cache[(name, R)] = f
    return _cache[(name, R)]


def mise_cases():
    """[(id, resolution0, depth, field name, threshold name)]: every pair x (the five fields x {0, logit(0.3)}, plus the two tie
    fields at -0.375); resolution0 = 1 with the refining fields only."""
    combos = [(f, t) for f in ('checker', 'sphere_rod_torus', 'ternary', 'sparse_tie0', 'nonfinite') for t in ('zero', 'logit03')]
    combos += [('sparse_tie375', 'tie375'), ('tie_checker', 'tie375')]
    out = []
    for res0, depth in MISE_PAIRS:
        for f, t in combos:
            if res0 == 1 and f not in REFINING:
                continue
            out.append(('%dx%d-%s-%s' % (res0, depth, f, t), res0, depth, f, t))
    return out


def mc_cases():
    """[(id, n, field name, threshold name)] of the marching-cubes tests; n = points per axis."""
    combos = [('checker', 'zero'), ('ternary', 'zero'), ('tie_checker', 'tie375'), ('tie_checker', 'logit03'), ('nonfinite', 'zero'),
              ('all_tie375', 'tie375'), ('all_above', 'zero')]
    return [('n%d-%s-%s' % (n, f, t), n, f, t) for n in MC_SIZES for f, t in combos]


def is_finite_case(field_name):
    return field_name != 'nonfinite'


def linear(idx, n):
    """[Q, 3] lattice points -> x-major linear indices int64 [Q]."""
    idx = np.asarray(idx, dtype=np.int64)
    return (idx[:, 0] * n + idx[:, 1]) * n + idx[:, 2]


def lock_step(values, res0, depth, thr):
    """Step a HostMISE over the lattice field ``values`` one round at a time -> (rounds, mise).  Per round:
      rows            sorted linear indices of the points queried
      flags_collect   the flags after the queried points became known (uint8 [n, n, n])
      flags_refine    the flags after the refinement marked the new points
      vox             every voxel level after the refinement
      new             the number of points the refinement marked (= the next round's query)"""
    from psnerf_amd.stage1.extracting import HostMISE
    mise = HostMISE(res0, depth, thr)
    n = mise.resolution + 1
    assert values.shape == (n, n, n) and values.dtype == np.float32
    rounds = []
    q = mise.query()
    while q.shape[0] != 0:
        assert len(rounds) < 64, 'the refinement does not terminate'
        mise.values[q[:, 0], q[:, 1], q[:, 2]] = values[q[:, 0], q[:, 1], q[:, 2]]
        mise.flags[q[:, 0], q[:, 1], q[:, 2]] = 2
        after_collect = mise.flags.copy()
        new = mise.refine()
        rounds.append(dict(rows=np.sort(linear(q, n)), flags_collect=after_collect, flags_refine=mise.flags.copy(),
                           vox=[v.copy() for v in mise.vox], new=int(new)))
        q = mise.query()
        assert q.shape[0] == new
    return rounds, mise


def sha256(array, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(array).astype(dtype)).tobytes()).hexdigest()


def on_lattice_point(vertices):
    """bool [V]: finite marching-cubes vertices (lattice units) all of whose coordinates are integers."""
    v = np.asarray(vertices, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.isfinite(v).all(axis=1) & (v == np.round(v)).all(axis=1)


def edges_defined(vertices):
    """Does mesh_fields.lattice_edges accept these vertices (every one has exactly one coordinate off the integers by > 1e-9)?"""
    v = np.asarray(vertices, dtype=np.float64)
    return bool(len(v)) and bool(np.isfinite(v).all()) and bool(((np.abs(v - np.round(v)) > 1e-9).sum(axis=1) == 1).all())


def mc_code(grid, thr):
    """What psn_mc_count must write, from the definition: (code uint8 [(n + 1)^3], vertices per run of 256 cells, triangles per
    run).  code = (which of the +x, +y, +z lattice edges at the cell's lower corner have ends that differ in value <= thr) |
    triangles of the cell's cube index << 3, on the grid padded with -1e6."""
    from psnerf_amd.stage1.extracting import CORNERS, PAD_VALUE, mc_table
    ntri_tab, _ = mc_table()
    P = np.pad(np.asarray(grid, dtype=np.float64), 1, 'constant', constant_values=PAD_VALUE)
    M = P.shape[0] - 1
    with np.errstate(invalid='ignore'):
        inside = P <= float(thr)
    cube = np.zeros((M, M, M), dtype=np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        cube |= inside[dx:dx + M, dy:dy + M, dz:dz + M].astype(np.int64) << c
    lower = inside[:M, :M, :M]
    vmask = (inside[1:, :M, :M] != lower) * 1 + (inside[:M, 1:, :M] != lower) * 2 + (inside[:M, :M, 1:] != lower) * 4
    ntri = ntri_tab[cube].astype(np.int64)
    code = (vmask | (ntri << 3)).astype(np.uint8).ravel()
    runs = (M ** 3 + 255) // 256
    pad = runs * 256 - M ** 3
    nv = np.concatenate([(vmask.ravel() & 1) + ((vmask.ravel() >> 1) & 1) + (vmask.ravel() >> 2), np.zeros(pad, dtype=np.int64)])
    nt = np.concatenate([ntri.ravel(), np.zeros(pad, dtype=np.int64)])
    return code, nv.reshape(runs, 256).sum(axis=1), nt.reshape(runs, 256).sum(axis=1)


# ---------------------------------------------------------------------------------------------- hole filling
FFILL_SIZES = [1, 2, 63, 64, 129, 130]
_SPECIALS = [-0.0, 1e-40, -1e-40, np.inf, -np.inf]


def ffill_grid(n):
    """A float32 [n, n, n] grid with holes (NaN) for psn_grid_ffill: 70 % random holes, -0.0 / denormal / infinite values among the
    known ones, and on top, as far as n has room for them (ffill_expectations says what survives until the z pass):
      z line (0, 0): all holes -- its first point is a hole and nothing ever fills it
      z line (0, 1): known only at z = 0 (value -0.0): every 64-point chunk behind the first is all holes
      z lines (0, 2), (0, 3): known only at z < 64 and z >= 128 (the value at z = 63 is a denormal): the middle chunk is all holes
      z line (1, 0): known only at z = 5 (-inf): a first point that stays a hole in front of a fill
      y runs in the plane x = 0 and x runs in the row y = n - 1: holes of every length 9 .. 17 starting at every q = 7 .. 10 (the
      strided kernel loads q = 1 .. 8, 9 .. 16, ... in batches of eight), each behind a known special value"""
    g = _rng('ffill', n)
    grid = g.randn(n, n, n).astype(np.float32)
    special = g.rand(n, n, n)
    for i, val in enumerate(_SPECIALS):
        grid[(special >= 0.02 * i) & (special < 0.02 * (i + 1))] = np.float32(val)
    grid[g.rand(n, n, n) < 0.7] = np.nan
    if n >= 38:                                        # the runs first: the constructed z lines below overwrite what they touch
        combos = [(q, length) for q in range(7, 11) for length in range(9, 18)]
        for c, (q, length) in enumerate(combos):
            k = 1 + c
            grid[0, q - 1, k] = np.float32(_SPECIALS[c % 5])
            grid[0, q:q + length, k] = np.nan
            grid[0, q + length, k] = 3.0
            grid[q - 1, n - 1, k] = np.float32(_SPECIALS[(c + 1) % 5])
            grid[q:q + length, n - 1, k] = np.nan
            grid[q + length, n - 1, k] = 4.0
    grid[0, 0, :] = np.nan
    if n >= 2:
        grid[0, 1, :] = np.nan
        grid[0, 1, 0] = np.float32(-0.0)
        grid[1, 0, :] = np.nan
    if n >= 7:
        grid[1, 0, 5] = -np.inf
    if n >= 129:
        for j in (2, 3):
            grid[0, j, :] = g.randn(n).astype(np.float32)
            grid[0, j, 64:128] = np.nan
            grid[0, j, 63] = np.float32(1e-40 * (1 if j == 2 else -1))
    grid[n - 1, n - 1, n - 1] = 1.5
    return grid


def ffill_before_z(grid):
    """The grid after the x and y passes of to_dense (what the z kernel starts from)."""
    g = grid.copy()
    n = g.shape[0]
    for axis in (0, 1):
        a = np.moveaxis(g, axis, 0)
        for q in range(1, n):
            hole = np.isnan(a[q])
            a[q][hole] = a[q - 1][hole]
    return g
