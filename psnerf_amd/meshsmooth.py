"""Mesh smoothing: Taubin's lambda | mu filter (G. Taubin, "A signal processing approach to fair surface design", 1995) over the vertex
rings of meshtopo.py, and the plain Laplacian it is built from.  A marching-cubes mesh of an occupancy grid carries the lattice's
staircase; a Laplacian step removes it and shrinks the object, the lambda | mu pair (a shrinking step, then an inflating one with
mu < -lambda) removes it and keeps the volume.  The extractor's lineage answers with refinement against the network
(``Extractor3D.refine_mesh``) and, everywhere else in practice, with this filter on the host through trimesh; the reference has none.

Two implementations of one definition, as in every mesh module:
  * CPU inputs -> ``host_smooth`` below, numpy float64 with every operation written out: it IS the definition.
  * device tensors (or ``device='cuda'``) -> csrc/meshtopo.hip: psn_topo_smooth_step, one launch per step over ping-pong buffers, one
    thread per vertex; the positions equal numpy's bit for bit.

Definition.  One step with factor s, per vertex v with ring w_0 < w_1 < ... of length n > 0 (meshtopo.host_rings), per axis:
    acc = +0.0;  acc += x[w_0];  acc += x[w_1]; ...;   m = acc / n;   x'[v] = x[v] + s (m - x[v])
  A vertex with an empty ring, or a pinned one, keeps its bits.  ``iterations`` = N runs N pairs of steps (s = lam, then s = mu);
  ``mu=None`` runs N plain Laplacian steps.  Refused with ValueError: lam outside (0, 1], mu not below -lam, negative iterations.
  ``pin='boundary'`` (the default) holds every vertex of an edge with count != 2 (a clipped mesh keeps its rim, non-manifold seams
  do not tear), ``pin=None`` holds nothing, a bool array [V] holds what it marks.  Vertices stay in their order, faces are untouched;
  incoming vertex normals are dropped (``normals='area'`` / ``'uniform'``: new ones by meshtopo's vertex normals).
  Report: n_pinned, n_isolated (vertices with an empty ring), iterations, max_displacement, mean_displacement (the length of
  x' - x per vertex, sqrt((dx dx + dy dy) + dz dz); 0.0 for no vertices), area / volume before and after (area_before, ...).  The
  displacement and area / volume values are sums whose order differs between the paths: report values, not compared bit for bit.
"""
import math

import numpy as np
import torch

from . import meshtopo
from .meshcore import Mesh, Phase, device_mesh, host_mesh, mesh_parts, on_device, to_numpy


def _check(iterations, lam, mu):
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 0:
        raise ValueError('smooth: iterations=%r (a non-negative integer)' % (iterations,))
    if not (0.0 < float(lam) <= 1.0):
        raise ValueError('smooth: lam=%r (in (0, 1])' % (lam,))
    if mu is not None and not (float(mu) < -float(lam) and math.isfinite(float(mu))):
        raise ValueError('smooth: mu=%r (below -lam = %r; None for the plain Laplacian)' % (mu, -float(lam)))
    return int(iterations), float(lam), (None if mu is None else float(mu))


def _factors(iterations, lam, mu):
    return [lam] * iterations if mu is None else [lam, mu] * iterations


def _pin_mask(pin, n_vertices):
    """pin given as an array -> bool numpy [V]."""
    mask = to_numpy(pin)
    mask = np.asarray(mask)
    if mask.dtype != np.bool_ or mask.reshape(-1).shape[0] != n_vertices:
        raise ValueError("smooth: pin must be 'boundary', None or a bool array [%d], got %s %s" % (n_vertices, mask.dtype, mask.shape))
    return mask.reshape(-1)


def _is_named_pin(pin):
    if pin is None or (isinstance(pin, str) and pin == 'boundary'):
        return True
    if isinstance(pin, str):
        raise ValueError("smooth: pin=%r ('boundary', None or a bool array)" % (pin,))
    return False


# ------------------------------------------------------------------------------------------------ host path: the definition
def host_step(x, ring_start, ring, held, s):
    """One step (module docstring): x float64 [V, 3], held bool [V] (pinned or isolated) -> x'.  np.add.at over the sorted directed
    pairs adds each vertex's neighbours one after the other in ascending order, from +0.0."""
    n = np.diff(ring_start)
    owner = np.repeat(np.arange(x.shape[0]), n)
    acc = np.zeros_like(x)
    np.add.at(acc, owner, x[ring])
    with np.errstate(all='ignore'):
        m = acc / np.where(n > 0, n, 1).astype(np.float64)[:, None]
        moved = x + s * (m - x)
    return np.where(held[:, None], x, moved)


def host_umbrella(vertices, ring_start, ring):
    """The mean over the vertices with a ring of |ring mean - x|: a roughness measure (tests and tools; not part of the filter)."""
    x = np.asarray(vertices, dtype=np.float64)
    n = np.diff(ring_start)
    acc = np.zeros_like(x)
    np.add.at(acc, np.repeat(np.arange(x.shape[0]), n), x[ring])
    has = n > 0
    d = acc[has] / n[has, None] - x[has]
    return float(np.sqrt((d * d).sum(axis=1)).mean()) if has.any() else 0.0


def _displacement(d):
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return (float(length.max()), float(length.mean())) if length.shape[0] else (0.0, 0.0)


def host_smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin='boundary'):
    """-> (vertices float64 [V, 3], report)."""
    iterations, lam, mu = _check(iterations, lam, mu)
    v, f, _ = host_mesh(vertices, faces)
    n_v = v.shape[0]
    named = _is_named_pin(pin)
    table = meshtopo.host_edges(f, n_v)
    ring_start, ring = meshtopo.host_rings(table['edges'], n_v)
    pinned = (table['vertex_open'] if pin == 'boundary' else np.zeros(n_v, dtype=bool)) if named else _pin_mask(pin, n_v)
    isolated = np.diff(ring_start) == 0
    held = pinned | isolated
    x = v
    for s in _factors(iterations, lam, mu):
        x = host_step(x, ring_start, ring, held, s)
    x = np.ascontiguousarray(x)
    before, after = meshtopo.host_measure_terms(v, f), meshtopo.host_measure_terms(x, f)
    d_max, d_mean = _displacement(x - v)
    return x, {'n_pinned': int(pinned.sum()), 'n_isolated': int(isolated.sum()), 'iterations': iterations, 'max_displacement': d_max,
               'mean_displacement': d_mean, 'area_before': float(before[0].sum()), 'volume_before': float(before[1].sum()),
               'area_after': float(after[0].sum()), 'volume_after': float(after[1].sum())}


# ------------------------------------------------------------------------------------------------ device path
def _device_smooth(v, f, iterations=10, lam=0.5, mu=-0.53, pin='boundary', events=None):
    """host_smooth on device tensors (float64 [V, 3], int64 [F, 3], contiguous) -> (vertices: a device tensor, report).  Host reads: the
    edge table's one, and one row of report values at the end."""
    from . import hip, ops
    iterations, lam, mu = _check(iterations, lam, mu)
    named = _is_named_pin(pin)
    ops._hit('MeshSmooth')
    n_v = v.shape[0]
    table = meshtopo._device_edges(f, n_v, events)
    ring_start, ring = meshtopo._device_rings(table['edges'], n_v, events)
    if named:
        pinned = table['vertex_open'] if pin == 'boundary' else None
    else:
        mask = pin if torch.is_tensor(pin) and pin.is_cuda and pin.dtype == torch.bool and pin.numel() == n_v else torch.from_numpy(_pin_mask(pin, n_v))
        pinned = mask.reshape(-1).to(device=v.device, dtype=torch.uint8).contiguous()
    with Phase(events, 'measures'):
        before = hip.topo_measures(v, f)
    with Phase(events, 'steps'):
        x, spare = v, None
        for s in _factors(iterations, lam, mu):
            out = hip.topo_smooth_step(x, ring_start, ring, pinned, s, out=spare)
            x, spare = out, (x if x is not v else None)               # (ping-pong; the caller's tensor is never written)
    with Phase(events, 'measures'):
        after = hip.topo_measures(x, f)
        d = x - v
        length = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        zero = before.new_zeros(())
        row = torch.stack([before[0], before[1], after[0], after[1], length.max() if n_v else zero, length.mean() if n_v else zero,
                           (pinned.sum(dtype=torch.float64) if pinned is not None else zero),
                           (ring_start[1:] == ring_start[:-1]).sum(dtype=torch.float64)]).tolist()
    return x, {'n_pinned': int(row[6]), 'n_isolated': int(row[7]), 'iterations': iterations, 'max_displacement': row[4],
               'mean_displacement': row[5], 'area_before': row[0], 'volume_before': row[1], 'area_after': row[2], 'volume_after': row[3]}


# ------------------------------------------------------------------------------------------------ public surface
def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, pin='boundary', normals=None, device=None):
    """``mesh``: anything with .vertices and .faces, or a tuple (vertices, faces[, normals]) -> (Mesh, report).  Device tensors, or
    ``device='cuda'``, take the device path (only the result is copied back); otherwise the host path.  Incoming vertex normals are
    dropped; ``normals`` = 'area' or 'uniform' forms new ones on the smoothed mesh (meshtopo.vertex_normals)."""
    if normals is not None:
        meshtopo._check_weight(normals)
    vertices, faces, _ = mesh_parts(mesh)
    if on_device(vertices, device):
        v, f, _ = device_mesh(vertices, faces, None, device)
        x, report = _device_smooth(v, f, iterations, lam, mu, pin)
        vn = None if normals is None else meshtopo._device_vertex_normals(x, f, normals, check=False).cpu().numpy()
        return Mesh(x.cpu().numpy(), f.cpu().numpy(), vertex_normals=vn), report
    v, f, _ = host_mesh(to_numpy(vertices), to_numpy(faces))
    x, report = host_smooth(v, f, iterations, lam, mu, pin)
    return Mesh(x, f, vertex_normals=None if normals is None else meshtopo.host_vertex_normals(x, f, normals)), report
