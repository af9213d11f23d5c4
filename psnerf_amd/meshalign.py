"""Registration of one mesh to another: trimmed point-to-plane ICP over a similarity, the step between exporting a mesh and
evaluating it.  get_chamfer_dist and evaluate_mesh presume that both meshes are in one frame; a scan in the scanner's frame and
millimetres, or a mesh exported in the normalised box of another run, is off by a similarity, and its Chamfer distance then measures
the misalignment.  ``align_mesh`` finds that similarity; ``apply`` moves a mesh by it.  The reference has no registration.

Two implementations of one definition, as in photostereo.py / meshbake.py:
  * numpy inputs -> the float64 functions below (``host_*``); they are the definition.
  * a ``MeshIndex`` or device tensors (or ``device='cuda'``) -> csrc/meshalign.hip (psn_align_transform, psn_align_dist,
    psn_align_sums) around ``MeshIndex.closest_point``.  Transformed points, closest points, distances, the trim's max_dist and the
    four row counts equal the definition bit for bit; the 37 sums are the same terms added in another (fixed) order.  The 7 x 7 solve
    and the update run on the host in float64 on both paths.  Two host reads per iteration: max_dist, and the 37 + 4 numbers.

The definition.
  Transform.  T = (s, R, t), T(x) = s (R x) + t: row i of R x is (R[i,0] x0 + R[i,1] x1) + R[i,2] x2, then the product with s, then
    the sum with t[i] (``host_transform``).  T^-1 = (1 / s, R^T, -T'(t)) with T' = (1 / s, R^T, 0), formed on the host.
  Rows.  The source samples x (``samples`` of them, drawn once) give the rows P = T(x), (Y, tri) = the closest point of P on the
    TARGET mesh and its triangle (host_closest_point / MeshIndex.closest_point), N = normalise(e1 x e2) of that triangle:
    (nx, ny, nz) = meshcore.face_cross, |n| = sqrt((nx nx + ny ny) + nz nz), N = n / |n|; a length that is not > 0 gives no normal
    (meshbake's rule).  ``symmetric`` adds the other direction without another index: the target samples y (as many, drawn after x)
    go into the source frame, x' = T^-1(y); (q, tri) = the closest point of x' on the SOURCE mesh; the row is P = T(q), Y = y,
    N = R n_tri, row i of R n as above.
  Distance.  d = |Y - P| = sqrt((dx dx + dy dy) + dz dz), (dx, dy, dz) = Y - P (``host_dist``).
  max_dist.  The k-th order statistic (from 0) of the d of ALL rows of the iteration, k = min(n, max(1, ceil(keep n))) - 1, a d that
    is not finite counting as +inf: an element of the data, never interpolated.  keep = 1: the largest.  The caller's ``max_dist``
    caps it.
  Gate.  A row is skipped as (1) NO TRIANGLE / NOT FINITE if tri is outside 0 .. F - 1 or a coordinate of P or Y is not finite, else
    as (2) ZERO NORMAL if |n| is not > 0, else as (3) BEYOND max_dist unless d <= max_dist (closed: a tie is kept).  Else it is USED.
  Sums, over the used rows (``host_sums``).  J = [P x N, N, P . N] with P x N = (P1 N2 - P2 N1, P2 N0 - P0 N2, P0 N1 - P1 N0) and
    P . N = (P0 N0 + P1 N1) + P2 N2; r = (N0 dx + N1 dy) + N2 dz.  The 37 doubles: J[a] J[b] for a <= b row by row (28), J[a] r (7),
    r r, and (dx dx + dy dy) + dz dz.  Four int64 counts: used, and the three skip counts in the order above.
  Update (``solve_update``, host, float64).  A = sum J J^T, b = sum J r; np.linalg.solve of the 7 x 7 system for 'similarity', of its
    leading 6 x 6 for 'rigid', of rows and columns 3 .. 5 for 'translation'; delta = (w, u, k), what a mode does not solve for is 0.
    dR = the Rodrigues rotation of w, ds = 1 + k, T <- (ds s, dR R, ds (dR t) + u): to first order T_new(x) = P + w x P + u + k P.
  Stop.  When |w| < tol and |u| < tol diag and |k| < tol (diag = the diagonal of the target's bounding box), or after
    ``max_iterations`` updates.  A singular system stops the iteration unconverged.
  Start.  init='moments': t = c_tgt - s R c_src with the area-weighted centroids c, R = the identity, s = sqrt(area_tgt / area_src)
    for 'similarity' and 1 otherwise; init=None: the identity; a 4 x 4 matrix: s = det^(1/3) of its 3 x 3 block, R = block / s (a
    block with det <= 0, a reflection, is refused).  ``starts``: a list of 3 x 3 rotations ('axes24': the 24 proper signed axis
    permutations, in the order of ``axes24``), each taken as R in the moments start (init=None: with t = 0, s = 1), run for
    ``coarse_iterations`` on ``coarse_samples`` samples of their own (drawn first); the start with the lowest rms goes on, ties to
    the lowest index.
  rms = sqrt(sum |Y - P|^2 / used) over the used rows, 'rms_plane' the same of r; NaN when no row is used.  The result's rms, used
    and max_dist are those of one last pass of the rows under the final transform.
"""
import itertools
import math

import numpy as np
import torch

from .meshcore import Mesh, Phase, face_areas, face_cross, mesh_parts, to_numpy
from .meshdist import MeshIndex, _HostMesh, _prepare

N_SUMS, N_COUNTS = 37, 4     # PSN_ALIGN_SUMS, PSN_ALIGN_COUNTS
MODES = ('rigid', 'similarity', 'translation')
_UPPER = [(a, b) for a in range(7) for b in range(a, 7)]


# ------------------------------------------------------------------------------------------------ host path: the definition
def host_transform(points, scale, rotation, translation):
    """T(x) = s (R x) + t in the stated order -> float64 [n, 3]."""
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    R, t, s = np.asarray(rotation, dtype=np.float64).reshape(3, 3), np.asarray(translation, dtype=np.float64).reshape(3), float(scale)
    with np.errstate(all='ignore'):
        return np.stack([s * ((R[i, 0] * x[:, 0] + R[i, 1] * x[:, 1]) + R[i, 2] * x[:, 2]) + t[i] for i in range(3)], axis=1)


def host_dist(P, Y):
    """|Y - P| per row in the stated order -> float64 [n]."""
    e = np.asarray(Y, dtype=np.float64).reshape(-1, 3) - np.asarray(P, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all='ignore'):
        return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def host_terms(P, Y, tri, vertices, faces, max_dist, rotation=None):
    """The rows' status and terms -> (status int64 [n]: 0 used, 1 no triangle / not finite, 2 zero normal, 3 beyond max_dist;
    terms float64 [n, 37], zero where the row is not used).  ``faces`` may name vertices outside 0 .. V - 1: such rows are status 1."""
    P, Y = np.asarray(P, dtype=np.float64).reshape(-1, 3), np.asarray(Y, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1)
    v, f = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not float(max_dist) >= 0.0:
        raise ValueError('meshalign: max_dist = %r (not negative, not NaN)' % (max_dist,))
    n = P.shape[0]
    status = np.zeros(n, dtype=np.int64)
    has_tri = (tri >= 0) & (tri < f.shape[0])
    t = f[np.where(has_tri, tri, 0)] if f.shape[0] else np.zeros((n, 3), dtype=np.int64)
    in_range = ((t >= 0) & (t < v.shape[0])).all(axis=1)
    ok1 = has_tri & np.isfinite(P).all(axis=1) & np.isfinite(Y).all(axis=1) & in_range
    t = np.where(in_range[:, None], t, 0)
    with np.errstate(all='ignore'):
        nx, ny, nz = face_cross(v, t)
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok2 = length > 0.0
        safe = np.where(ok2, length, 1.0)
        N = [nx / safe, ny / safe, nz / safe]
        if rotation is not None:
            R = np.asarray(rotation, dtype=np.float64).reshape(3, 3)
            N = [(R[i, 0] * N[0] + R[i, 1] * N[1]) + R[i, 2] * N[2] for i in range(3)]
        e = [Y[:, i] - P[:, i] for i in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        ok3 = np.sqrt(d2) <= float(max_dist)
        status = np.where(~ok1, 1, np.where(~ok2, 2, np.where(~ok3, 3, 0))).astype(np.int64)
        p = [P[:, i] for i in range(3)]
        J = [p[1] * N[2] - p[2] * N[1], p[2] * N[0] - p[0] * N[2], p[0] * N[1] - p[1] * N[0], N[0], N[1], N[2],
             (p[0] * N[0] + p[1] * N[1]) + p[2] * N[2]]
        r = (N[0] * e[0] + N[1] * e[1]) + N[2] * e[2]
        terms = np.stack([J[a] * J[b] for a, b in _UPPER] + [J[a] * r for a in range(7)] + [r * r, d2], axis=1)
    used = status == 0
    return status, np.where(used[:, None], terms, 0.0)


def host_sums(P, Y, tri, vertices, faces, max_dist, rotation=None):
    """The 37 sums and the four counts of the rows (module docstring) -> (sums float64 [37], counts int64 [4])."""
    status, terms = host_terms(P, Y, tri, vertices, faces, max_dist, rotation)
    return terms[status == 0].sum(axis=0), np.bincount(status, minlength=N_COUNTS).astype(np.int64)


# ------------------------------------------------------------------------------------------------ transforms (host values on both paths)
def to_matrix(T):
    s, R, t = T
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = float(s) * np.asarray(R, dtype=np.float64), t
    return m


def from_matrix(matrix):
    """A 4 x 4 similarity -> (s, R, t).  A 3 x 3 block with det <= 0 (a reflection, or a collapse), a block that is not s x a rotation
    or a last row other than (0, 0, 0, 1) is refused."""
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError('meshalign: a finite 4 x 4 matrix expected, got %s' % (m.shape,))
    if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError('meshalign: the last row of the matrix is %s, not (0, 0, 0, 1)' % (m[3].tolist(),))
    det = float(np.linalg.det(m[:3, :3]))
    if not det > 0.0:
        raise ValueError('meshalign: the matrix has determinant %g: a reflection (or a collapse) is no proper similarity and would turn '
                         'the mesh inside out' % det)
    s = det ** (1.0 / 3.0)
    R = m[:3, :3] / s
    if float(np.abs(R @ R.T - np.eye(3)).max()) > 1e-6:
        raise ValueError('meshalign: the 3 x 3 block is not a scale times a rotation (|R R^T - 1| = %.3g)' % float(np.abs(R @ R.T - np.eye(3)).max()))
    return s, R, m[:3, 3].copy()


def inverse(T):
    s, R, t = T
    si, Ri = 1.0 / float(s), np.ascontiguousarray(np.asarray(R).T)
    return si, Ri, -host_transform(np.asarray(t)[None], si, Ri, np.zeros(3))[0]


def rodrigues(w):
    """The rotation by |w| about w / |w| -> float64 [3, 3]; the identity for w = 0."""
    w = np.asarray(w, dtype=np.float64)
    theta = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if theta == 0.0:
        return np.eye(3)
    k = w / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(theta) * K + (2.0 * math.sin(0.5 * theta) ** 2) * (K @ K)


def solve_update(sums, mode):
    """The 37 sums -> delta = (w [3], u [3], k) of the mode, or None when the system is singular or not finite."""
    sums = np.asarray(sums, dtype=np.float64)
    A = np.zeros((7, 7))
    for i, (a, b) in enumerate(_UPPER):
        A[a, b] = A[b, a] = sums[i]
    rhs = sums[28:35]
    idx = {'similarity': list(range(7)), 'rigid': list(range(6)), 'translation': [3, 4, 5]}[mode]
    delta = np.zeros(7)
    try:
        delta[idx] = np.linalg.solve(A[np.ix_(idx, idx)], rhs[idx])
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(delta).all():
        return None
    return delta[0:3], delta[3:6], float(delta[6])


def compose_update(T, delta):
    s, R, t = T
    w, u, k = delta
    dR, ds = rodrigues(w), 1.0 + k
    return ds * float(s), dR @ np.asarray(R), ds * (dR @ np.asarray(t)) + u


def axes24():
    """The 24 proper rotations that permute the axes with signs, the identity first: row i of the matrix is sign[i] e_perm[i], over
    itertools.permutations(range(3)) and itertools.product((1, -1), repeat=3) in their orders, those with determinant +1."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0.0:
                out.append(R)
    return out


# ------------------------------------------------------------------------------------------------ one code path over both
def _is_device(mesh):
    return isinstance(mesh, MeshIndex)


def _transform(mesh, points, T):
    if _is_device(mesh):
        from . import hip
        return hip.align_transform(points, T[0], T[1], T[2])
    return host_transform(points, *T)


def _dist(mesh, P, Y):
    if _is_device(mesh):
        from . import hip
        return hip.align_dist(P, Y)
    return host_dist(P, Y)


def _sums(mesh, P, Y, tri, max_dist, rotation):
    """The sums of rows whose normals are those of ``mesh`` -> (sums [37], counts [4]) on the host."""
    if _is_device(mesh):
        from . import hip
        sums, counts, _ = hip.align_sums(P, Y, tri, mesh.vertices, mesh.faces, max_dist, rotation)
        both = torch.cat([sums, counts.to(torch.float64)]).tolist()     # (one read; a count below 2^53 is exact as a double)
        return np.asarray(both[:N_SUMS]), np.asarray(both[N_SUMS:], dtype=np.float64).astype(np.int64)
    return host_sums(P, Y, tri, mesh.vertices, mesh.faces, max_dist, rotation)


def quantile_index(keep, n):
    return min(n, max(1, int(math.ceil(float(keep) * n)))) - 1


def _max_dist(dists, keep, cap):
    """The trim's max_dist of the iteration's row distances (a list of arrays or device tensors) -> float."""
    if torch.is_tensor(dists[0]):
        d = torch.cat(dists) if len(dists) > 1 else dists[0]
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
        value = float(torch.kthvalue(d, quantile_index(keep, d.numel()) + 1).values)
    else:
        d = np.concatenate(dists)
        d = np.where(np.isfinite(d), d, np.inf)
        k = quantile_index(keep, d.size)
        value = float(np.partition(d, k)[k])
    return value if cap is None else min(value, float(cap))


def rows(src, tgt, x, y, T, symmetric=False, phases=None):
    """The rows of one iteration under T -> a list of (P, Y, tri, mesh whose normals are meant, rotation of the normal or None)."""
    with Phase(phases, 'transform'):
        P = _transform(tgt, x, T)
    with Phase(phases, 'closest_point'):
        Y, _, tri = tgt.closest_point(P)
    out = [(P, Y, tri, tgt, None)]
    if symmetric:
        with Phase(phases, 'transform'):
            xs = _transform(src, y, inverse(T))
        with Phase(phases, 'closest_point'):
            q, _, tri2 = src.closest_point(xs)
        with Phase(phases, 'transform'):
            P2 = _transform(src, q, T)
        out.append((P2, y, tri2, src, np.asarray(T[1], dtype=np.float64)))
    return out


def align_step(src, tgt, x, y, T, keep=0.9, max_dist=None, symmetric=False, phases=None):
    """One pass of the rows under T = (s, R, t): ``src`` / ``tgt`` both MeshIndex (x, y device tensors) or both host meshes ->
    dict(sums float64 [37], counts int64 [4], max_dist, used, rms, rms_plane).  ``phases``: a list that receives the HIP-event
    brackets of the device steps (tools/bench_align.py)."""
    rs = rows(src, tgt, x, y, T, symmetric, phases)
    with Phase(phases, 'quantile'):
        limit = _max_dist([_dist(m, P, Y) for P, Y, _, m, _ in rs], keep, max_dist)
    sums, counts = np.zeros(N_SUMS), np.zeros(N_COUNTS, dtype=np.int64)
    with Phase(phases, 'sums'):
        for P, Y, tri, m, rot in rs:       # (the two directions' sums are added on the host, forward first)
            s_, c_ = _sums(m, P, Y, tri, limit, rot)
            sums, counts = sums + s_, counts + c_
    used = int(counts[0])
    rms = math.sqrt(sums[36] / used) if used else float('nan')
    rms_plane = math.sqrt(sums[35] / used) if used else float('nan')
    return {'sums': sums, 'counts': counts, 'max_dist': limit, 'used': used, 'rms': rms, 'rms_plane': rms_plane}


def _iterate(src, tgt, x, y, T, mode, keep, max_dist, symmetric, max_iterations, tol, diag):
    history, converged = [], False
    for _ in range(int(max_iterations)):
        step = align_step(src, tgt, x, y, T, keep, max_dist, symmetric)
        history.append({'used': step['used'], 'rms': step['rms'], 'rms_plane': step['rms_plane'], 'max_dist': step['max_dist'],
                        'skipped': [int(c) for c in step['counts'][1:]], 'matrix': to_matrix(T),
                        'transform': (float(T[0]), np.array(T[1], dtype=np.float64), np.array(T[2], dtype=np.float64))})
        delta = solve_update(step['sums'], mode) if step['used'] else None
        if delta is None:
            break
        T = compose_update(T, delta)
        w, u, k = delta
        if np.linalg.norm(w) < tol and np.linalg.norm(u) < tol * diag and abs(k) < tol:
            converged = True
            break
    return T, history, converged


def _moments(mesh):
    """(area, area-weighted centroid [3]) of a mesh on either path, as host values."""
    v, f = mesh.vertices, mesh.faces
    area = face_areas(v, f)
    centre = (v[f[:, 0]] + v[f[:, 1]] + v[f[:, 2]]) / 3.0
    if torch.is_tensor(area):
        head = torch.cat([area.sum().reshape(1), (area[:, None] * centre).sum(0)]).tolist()
    else:
        head = [float(area.sum())] + (area[:, None] * centre).sum(0).tolist()
    total = head[0]
    if not total > 0.0:
        raise ValueError('meshalign: a mesh of area %g has no centroid' % total)
    return total, np.asarray(head[1:4]) / total


def _diag(mesh):
    if _is_device(mesh):
        lo, hi = np.asarray(mesh.lo, dtype=np.float64), np.asarray(mesh.hi, dtype=np.float64)
    else:
        lo, hi = mesh.vertices.min(axis=0), mesh.vertices.max(axis=0)
    return float(np.sqrt(((hi - lo) ** 2).sum()))


def _start(src, tgt, mode, init, rotation=None):
    R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
    if rotation is not None and (not np.linalg.det(R) > 0.0 or float(np.abs(R @ R.T - np.eye(3)).max()) > 1e-6):
        raise ValueError('meshalign: a start that is no proper rotation (det %g) is refused' % float(np.linalg.det(R)))
    if init is None:
        return 1.0, R, np.zeros(3)
    area_s, c_s = _moments(src)
    area_t, c_t = _moments(tgt)
    s = math.sqrt(area_t / area_s) if mode == 'similarity' else 1.0
    return s, R, c_t - s * (R @ c_s)


def _samples(mesh, count, rng):
    return mesh.sample_surface(int(count), rng)[0]


def align_mesh(source, target, mode='rigid', samples=20000, keep=0.9, symmetric=False, max_iterations=50, tol=1e-10, init='moments',
               starts=None, rng=None, device=None, max_dist=None, coarse_iterations=8, coarse_samples=2000):
    """Register the mesh ``source`` to ``target`` (anything with ``.vertices`` and ``.faces``, a MeshIndex, or a tuple) by the rule of
    the module docstring -> dict(matrix float64 [4, 4] taking source to target, scale, rotation [3, 3], translation [3], rms,
    rms_plane, used, max_dist, iterations, converged, history: per iteration dict(used, rms, rms_plane, max_dist, skipped, matrix and
    transform = (s, R, t): what the rows were formed under), start: the index of the chosen start or None).  Device tensors, a MeshIndex or
    ``device='cuda'`` take the device path, otherwise the numpy host path.  ``rng``: np.random.RandomState (default: the global
    np.random); the draws are the coarse source (and, symmetric, target) samples when there are ``starts``, then the source (and
    target) samples."""
    if mode not in MODES:
        raise ValueError('align_mesh: mode %r (%s)' % (mode, ', '.join(MODES)))
    if not 0.0 < float(keep) <= 1.0:
        raise ValueError('align_mesh: keep = %r (in (0, 1])' % (keep,))
    if max_dist is not None and not float(max_dist) >= 0.0:
        raise ValueError('align_mesh: max_dist = %r (not negative, not NaN)' % (max_dist,))
    if int(samples) < 1:
        raise ValueError('align_mesh: samples = %r (at least 1)' % (samples,))
    src, tgt = _prepare(source, device, 'source'), _prepare(target, device, 'target')
    if _is_device(src) != _is_device(tgt):
        raise ValueError('align_mesh: source and target must both be on the device or both on the host')
    diag = _diag(tgt)
    start = None
    if starts is not None:
        if init is not None and not (isinstance(init, str) and init == 'moments'):
            raise ValueError('align_mesh: starts go with init=\'moments\' or init=None')
        rotations = axes24() if isinstance(starts, str) and starts == 'axes24' else [np.asarray(R, dtype=np.float64) for R in starts]
        if not rotations:
            raise ValueError('align_mesh: an empty list of starts')
        cx = _samples(src, coarse_samples, rng)
        cy = _samples(tgt, coarse_samples, rng) if symmetric else None
        best = None
        for i, R0 in enumerate(rotations):
            T0, _, _ = _iterate(src, tgt, cx, cy, _start(src, tgt, mode, init, R0), mode, keep, max_dist, symmetric, coarse_iterations,
                                tol, diag)
            score = align_step(src, tgt, cx, cy, T0, keep, max_dist, symmetric)['rms']
            if not math.isnan(score) and (best is None or score < best[0]):      # (strict: ties go to the lowest index)
                best = (score, i, T0)
        if best is None:
            raise ValueError('align_mesh: no start used a single row')
        start, T = best[1], best[2]
    elif init is None or (isinstance(init, str) and init == 'moments'):
        T = _start(src, tgt, mode, init)
    elif isinstance(init, str):
        raise ValueError('align_mesh: init %r (\'moments\', None or a 4 x 4 matrix)' % (init,))
    else:
        T = from_matrix(init)
    x = _samples(src, samples, rng)
    y = _samples(tgt, samples, rng) if symmetric else None
    T, history, converged = _iterate(src, tgt, x, y, T, mode, keep, max_dist, symmetric, max_iterations, tol, diag)
    last = align_step(src, tgt, x, y, T, keep, max_dist, symmetric)
    return {'matrix': to_matrix(T), 'scale': float(T[0]), 'rotation': np.asarray(T[1]), 'translation': np.asarray(T[2]), 'rms': last['rms'],
            'rms_plane': last['rms_plane'], 'used': last['used'], 'max_dist': last['max_dist'], 'iterations': len(history),
            'converged': converged, 'history': history, 'start': start, 'mode': mode}


def moved(mesh, matrix):
    """A prepared mesh (MeshIndex or its host twin) moved by a 4 x 4 similarity -> a new one of the same kind; on the device the
    vertices never leave it, and the index is built once for the new position."""
    T = from_matrix(matrix)
    if _is_device(mesh):
        return MeshIndex(_transform(mesh, mesh.vertices, T), mesh.faces, name='moved mesh')
    return _HostMesh(host_transform(mesh.vertices, *T), mesh.faces, 'moved mesh')


def apply(matrix, mesh):
    """Move a mesh by a 4 x 4 similarity (align_mesh's ``matrix``) -> Mesh: the vertices by T (device tensors: psn_align_transform),
    the vertex normals, where there are any, by its rotation; the faces unchanged, since a proper similarity keeps the winding.  A
    matrix with a reflection is refused."""
    T = from_matrix(matrix)
    v, f, normals = mesh_parts(mesh)
    if torch.is_tensor(v) and v.is_cuda:
        from . import hip
        moved = to_numpy(hip.align_transform(v.to(torch.float64).reshape(-1, 3).contiguous(), *T))
    else:
        moved = host_transform(to_numpy(v), *T)
    if normals is not None:
        normals = host_transform(np.asarray(to_numpy(normals), dtype=np.float64), 1.0, T[1], np.zeros(3))
    return Mesh(moved, np.array(to_numpy(f), dtype=np.int64, copy=True), vertex_normals=normals)
