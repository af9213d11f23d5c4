"""Mesh extraction from the stage-1 occupancy field with the reference's ``Extractor3D`` interface
(stage1/model/extracting.py:15-235; utils/libmise/mise.pyx; utils/libmcubes/marchingcubes.h:23-193).

Two implementations of one definition:
  * device tensors -> csrc/mesh.hip.  Value grid, point flags and voxel states stay on the device for the whole extraction; a
    round is psn_mise_collect (pending points -> compact list), the evaluation of that list scattered into the grid, and
    psn_mise_refine (split the active leaves, mark the new points); the host reads one 8-byte count per round.  Then
    psn_grid_ffill (to_dense), psn_mc_count / psn_mc_emit.  A ``NeuralNetwork`` whose geometry net the lean register-resident
    engine holds is evaluated by that engine straight from the list (fused.pack_geo_logit); any other callable with the
    reference's signature is called in ``points_batch_size`` batches.
  * CPU tensors -> the vectorised numpy functions below (``host_*``), which are also the pinned restatement of the semantics
    the device path is tested against.

Semantics (restated from the reference, see the functions for the line numbers):
  value(p) = -logit(p) = model(p[None], None, return_logits=True); iso value log(t) - log(1 - t) in double.
  Grid point (i, j, k) of the (R + 1)^3 lattice, R = resolution0 << upsampling_steps, is the point
  box_size * ((float)i / (float)R - 0.5f) per axis in float32, box_size = 2 + padding.
  MISE: leaf voxels that see a known value >= iso and one <= iso in their closed cube are split until nothing new appears
  (a least fixed point: the order of the tests within a round does not change the final set of evaluated points).
  to_dense: holes take their predecessor's value along x, then y, then z.  Marching cubes runs on the grid padded with -1e6,
  with the case table of csrc/mc_table.h (tools/gen_mc_table.py); vertices are float64.
Clean-up (not in the reference; opt-in): ``Extractor3D(..., keep_components=K, min_component_faces=N)`` keeps the K largest
  connected components of the extracted mesh among those with at least N faces (psnerf_amd/meshclean.py; on the device
  csrc/meshclean.hip, applied to the device tensors before the copy-back and before the normals are estimated).  With both at
  their defaults (None, 0) the extraction is bit for bit what it was.
Simplification (the lineage's ``simplify_nfaces``, which UNISURF and the reference dropped with its native library; opt-in):
  ``Extractor3D(..., simplify_nfaces=N)`` reduces the mesh to at most N faces by quadric vertex clustering (psnerf_amd/meshsimplify.py;
  on the device csrc/meshsimplify.hip), after the clean-up and before the copy-back and the normals.  None (the default) = off.
Smoothing (not in the reference; opt-in): ``Extractor3D(..., smooth_iterations=N, smooth_lambda=0.5, smooth_mu=-0.53)`` runs N
  lambda | mu pairs of Taubin's filter over the vertex rings (psnerf_amd/meshsmooth.py; on the device csrc/meshtopo.hip), with the rim
  and non-manifold seams pinned, after the clean-up and before the simplification, so that the quadrics see the smoothed face planes.
  None (the default) = off: no launch, tensor or byte of the extraction changes.
Carving (the reference's ``mask_loader``, extracting.py:120-127, with the project's projection; opt-in): ``Extractor3D(..., carve=hull)``
  with a ``psnerf_amd.hull.VisualHull`` sets the dense grid to -30 where a lattice point lies in no image, or where some image that
  contains it shows background in its dilated mask: after to_dense (and in the upsampling_steps = 0 branch), before ``clip``.  On the
  device grid csrc/hull.hip:psn_hull_grid, on the host path's numpy grid the definition (hull.host_carve_grid).  None (the default) =
  off: every launch, stat and result is what it was.
Vertex refinement (extracting.py:237-323): ``Extractor3D.refine_mesh(mesh, steps=N)`` / tools/refine_mesh.py run the reference's
  RMSprop refinement of the vertices against the field (``refine_loss`` / ``refine_vertices`` below).  The reference's method calls
  ``self.model.decoder``, which its own NeuralNetwork does not have, so it cannot run there; it is restated with
  ``self.model(p, None, only_occupancy=True)``, the reading ``estimate_normals`` already takes.  Two implementations of one definition:
  any differentiable callable through autograd.grad(create_graph=True) (any dtype; the host path, with oracle.stage1.NeuralNetwork),
  and for a ``NeuralNetwork`` on the device ONE ops.GeoFieldFused call per step whose backward returns d / dp (csrc/geo_dp.hip).
Not implemented, and refused loudly:
  ``refinement_step > 0`` as a CONSTRUCTOR argument of generate_mesh / generate_from_latent (every shipped config uses 0): call
    ``refine_mesh`` on the extracted mesh, or tools/refine_mesh.py on the written file;
  ``mask_loader`` (extracting.py:326-377): the reference's filter_points assumes UNISURF's world -> NDC matrices, while the
    reference's own loader supplies camera-to-world poses and a pixel-unit K (stage1/dataloading/dataset.py:125-127), so a faithful
    port would carve with the wrong projection on this project's data.  ``carve=VisualHull.from_loader(mask_loader)`` is the same rule
    with the projection of this project's camera.
"""
import os
import re
import time

import numpy as np
import torch

from ..meshcore import Mesh, Phase

PAD_VALUE = -1e6
_HERE = os.path.dirname(os.path.abspath(__file__))
_TABLE = None

# the lattice edge cube edge e lies on: owning corner offset (dx, dy, dz) and axis
EDGE_OWNER = np.array([[0, 0, 0, 0], [1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [1, 0, 1, 1],
                       [0, 1, 1, 0], [0, 0, 1, 1], [0, 0, 0, 2], [1, 0, 0, 2], [1, 1, 0, 2], [0, 1, 0, 2]], dtype=np.int64)
CORNERS = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.int64)


def mc_table():
    """(n_tri uint8 [256], tri int8 [256, 16]) parsed from csrc/mc_table.h -- the one table both paths use."""
    global _TABLE
    if _TABLE is None:
        text = open(os.path.join(_HERE, '..', 'csrc', 'mc_table.h')).read()
        text = re.sub(r'//[^\n]*', '', text)
        m1 = re.search(r'PSN_MC_NTRI\[256\]\s*=\s*\{(.*?)\};', text, re.S)
        m2 = re.search(r'PSN_MC_TRI\[256\]\[16\]\s*=\s*\{(.*)\};', text, re.S)
        ntri = np.array([int(x) for x in re.findall(r'-?\d+', m1.group(1))], dtype=np.uint8)
        tri = np.array([int(x) for x in re.findall(r'-?\d+', m2.group(1))], dtype=np.int8).reshape(256, 16)
        assert ntri.shape == (256,) and all(int((tri[c] >= 0).sum()) == 3 * int(ntri[c]) for c in range(256))
        _TABLE = (ntri, tri)
    return _TABLE


def iso_value(threshold):
    """extracting.py:83: the logit of the occupancy threshold, in double."""
    return float(np.log(threshold) - np.log(1. - threshold))


def grid_points_host(idx, resolution, box_size):
    """extracting.py:105-108 for integer lattice points [Q, 3] -> float32 points [Q, 3]."""
    p = torch.as_tensor(np.asarray(idx)).to(torch.float32)
    p = p / np.float32(resolution)
    return np.float32(box_size) * (p - 0.5)


# ------------------------------------------------------------------------------------------------ host path: MISE
class HostMISE(object):
    """mise.pyx restated on dense numpy arrays: ``flags`` [n, n, n] (0 no grid point, 1 pending, 2 known), ``values`` float32
    [n, n, n] (NaN = hole), one state array per level < depth (0 absent, 1 leaf, 2 split).  query() / update() as the reference;
    a round tests the levels finest first, so voxels created in a round are first tested in the next one."""

    def __init__(self, resolution0, depth, threshold):
        self.resolution0, self.depth, self.threshold = int(resolution0), int(depth), float(threshold)
        self.resolution = self.resolution0 << self.depth
        n = self.resolution + 1
        self.values = np.full((n, n, n), np.nan, dtype=np.float32)
        self.flags = np.zeros((n, n, n), dtype=np.uint8)
        s = 1 << self.depth
        self.flags[::s, ::s, ::s] = 1                                              # mise.pyx:76-86
        self.vox = [np.zeros((self.resolution0 << l,) * 3, dtype=np.uint8) for l in range(self.depth)]
        if self.depth > 0:
            self.vox[0][:] = 1                                                     # mise.pyx:58-73

    def query(self):
        """mise.pyx:107-129: the grid points without a value, int64 [Q, 3]."""
        return np.argwhere(self.flags == 1).astype(np.int64)

    def update(self, points, values):
        """mise.pyx:88-105: set the values, then subdivide the active voxels."""
        points = np.asarray(points)
        self.values[points[:, 0], points[:, 1], points[:, 2]] = np.asarray(values, dtype=np.float32)
        self.flags[points[:, 0], points[:, 1], points[:, 2]] = 2
        self.refine()

    @staticmethod
    def _window_any(a, s):
        """any() over the closed windows [i s, i s + s] along every axis of a boolean (m s + 1)^3 array -> [m, m, m]."""
        for axis in range(3):
            a = np.moveaxis(a, axis, 0)
            m = (a.shape[0] - 1) // s
            body = a[:-1].reshape((m, s) + a.shape[1:]).any(axis=1)
            a = np.moveaxis(body | a[s::s], 0, axis)
        return a

    def refine(self):
        """mise.pyx:185-282.  Returns the number of grid points that became pending."""
        known = self.flags == 2
        v = self.values.astype(np.float64)
        with np.errstate(invalid='ignore'):
            ge = known & (v >= self.threshold)                                     # mise.pyx:216-219, both non-strict
            le = known & (v <= self.threshold)
        new = 0
        for l in range(self.depth - 1, -1, -1):
            s = 1 << (self.depth - l)
            active = (self.vox[l] == 1) & self._window_any(ge, s) & self._window_any(le, s)
            if not active.any():
                continue
            self.vox[l][active] = 2
            if l + 1 < self.depth:
                child = np.repeat(np.repeat(np.repeat(active, 2, 0), 2, 1), 2, 2)
                self.vox[l + 1][child] = 1
            h = s >> 1
            base = np.argwhere(active) * s
            for d in range(27):                                                    # mise.pyx:269-281
                q = base + np.array([d // 9, (d // 3) % 3, d % 3]) * h
                f = self.flags[q[:, 0], q[:, 1], q[:, 2]]
                q = q[f == 0]
                new += int(len(np.unique(q, axis=0))) if len(q) else 0
                self.flags[q[:, 0], q[:, 1], q[:, 2]] = 1
        return new

    def to_dense(self):
        return host_ffill(self.values.copy())


def host_ffill(grid):
    """mise.pyx:143-164: holes (NaN) take their predecessor's value along x, then along y, then along z.  In place."""
    n = grid.shape[0]
    for axis in range(3):
        g = np.moveaxis(grid, axis, 0)
        for q in range(1, n):
            hole = np.isnan(g[q])
            g[q][hole] = g[q - 1][hole]
    return grid


# ------------------------------------------------------------------------------------------------ host path: marching cubes
def host_marching_cubes(grid, threshold):
    """marchingcubes.h:23-193 on ``grid`` padded with -1e6 (extracting.py:170-171) -> (vertices float64 [V, 3] in units of the
    padded lattice, faces int64 [F, 3]).  Vertices ascending by (owning lattice point x-major, axis), faces by (cell x-major,
    table order).  The iso crossing is formed in double as marchingcubes.cpp:290-297 does, x edges from their upper end
    (marchingcubes.h:78), y and z edges from their lower end (:84, :90)."""
    ntri_tab, tri_tab = mc_table()
    thr = float(threshold)
    P = np.pad(np.asarray(grid, dtype=np.float64), 1, 'constant', constant_values=PAD_VALUE)
    N = P.shape[0]
    M = N - 1
    inside = P <= thr
    cube = np.zeros((M, M, M), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = CORNERS[c]
        cube |= inside[dx:dx + M, dy:dy + M, dz:dz + M].astype(np.int64) << c
    b0 = cube & 1
    vmask = (((cube >> 1) & 1) != b0) * 1 + (((cube >> 3) & 1) != b0) * 2 + (((cube >> 4) & 1) != b0) * 4
    vcount = ((vmask & 1) + ((vmask >> 1) & 1) + ((vmask >> 2) & 1)).ravel()
    voff = np.cumsum(vcount) - vcount
    n_v = int(vcount.sum())
    vertices = np.zeros((n_v, 3), dtype=np.float64)
    vm = vmask.ravel()
    for a in range(3):
        sel = np.nonzero((vm >> a) & 1)[0]
        p = np.stack(np.unravel_index(sel, (M, M, M)), axis=1)
        q = p.copy()
        q[:, a] += 1
        f0, fq = P[p[:, 0], p[:, 1], p[:, 2]], P[q[:, 0], q[:, 1], q[:, 2]]
        lo, hi = p[:, a].astype(np.float64), q[:, a].astype(np.float64)
        (x1, x2, f1, f2) = (hi, lo, fq, f0) if a == 0 else (lo, hi, f0, fq)
        with np.errstate(invalid='ignore'):                                        # (infinite ends: inf / inf = NaN, as on the device)
            pos = (x2 - x1) * (thr - f1) / (f2 - f1) + x1
        at = voff[sel] + (((vm[sel] & ((1 << a) - 1)) & 1) + ((vm[sel] & ((1 << a) - 1)) >> 1))
        out = p.astype(np.float64)
        out[:, a] = pos
        vertices[at] = out
    ntri = ntri_tab[cube.ravel()].astype(np.int64)
    toff = np.cumsum(ntri) - ntri
    faces = np.zeros((int(ntri.sum()), 3), dtype=np.int64)
    cflat = cube.ravel()
    for t in range(int(ntri.max()) if ntri.size else 0):
        sel = np.nonzero(ntri > t)[0]
        p = np.stack(np.unravel_index(sel, (M, M, M)), axis=1)
        for c in range(3):
            e = tri_tab[cflat[sel], 3 * t + c].astype(np.int64)
            o = p + EDGE_OWNER[e, :3]
            oc = (o[:, 0] * M + o[:, 1]) * M + o[:, 2]
            low = vm[oc] & ((1 << EDGE_OWNER[e, 3]) - 1)
            faces[toff[sel] + t, c] = voff[oc] + (low & 1) + (low >> 1)
    return vertices, faces


def to_world(vertices, n, box_size):
    """extracting.py:175-181 for vertices in units of the padded lattice (the reference's own +0.5 is cancelled by its -0.5)."""
    v = vertices - 1.0
    v = v / np.array([n - 1, n - 1, n - 1], dtype=np.float64)
    return box_size * (v - 0.5)


# ------------------------------------------------------------------------------------------------ the extractor
class Extractor3D(object):
    """extracting.py:15-52, same constructor and methods."""

    def __init__(self, model, points_batch_size=100000, threshold=0.5, refinement_step=0, device=None, resolution0=16,
                 upsampling_steps=3, with_normals=False, padding=0.4, refine_max_faces=10000, keep_components=None,
                 min_component_faces=0, simplify_nfaces=None, carve=None, smooth_iterations=None, smooth_lambda=0.5, smooth_mu=-0.53):
        if device is None and isinstance(model, torch.nn.Module):
            device = next(model.parameters()).device   # (the reference leaves the model where it is; so do we, and follow it)
        self.model = model.to(device) if (model is not None and hasattr(model, 'to')) else model
        self.points_batch_size = points_batch_size
        self.refinement_step = refinement_step
        self.threshold = threshold
        self.device = torch.device(device) if device is not None else torch.device('cpu')
        self.resolution0 = resolution0
        self.upsampling_steps = upsampling_steps
        self.with_normals = with_normals
        self.padding = padding
        self.refine_max_faces = refine_max_faces
        # clean-up (meshclean.py): keep the K largest connected components among those with at least N faces; (None, 0) = off
        self.keep_components = keep_components
        self.min_component_faces = min_component_faces
        # simplification (meshsimplify.py): quadric vertex clustering to at most this many faces, after the clean-up; None = off
        self.simplify_nfaces = simplify_nfaces
        # smoothing (meshsmooth.py): this many lambda | mu pairs (mu = None: plain Laplacian steps) with the rim and non-manifold seams
        # pinned, after the clean-up and before the simplification; None = off
        self.smooth_iterations = smooth_iterations
        self.smooth_lambda = smooth_lambda
        self.smooth_mu = smooth_mu
        # carving (hull.py): a VisualHull whose dilated masks carve the dense grid before marching cubes; None = off
        self.carve = carve
        self.last_grid = None   # the dense value grid of the last generate_* call (device tensor or numpy array)
        self.phase_events = None  # a list: (phase, start event, end event) of the device phases are appended (measurement runs)
        self.last_known = None  # which of its points were evaluated (bool, same shape; None without upsampling: all of them)

    # -- reference API ------------------------------------------------------------------------------------------------
    def generate_mesh(self, data=None, return_stats=True, mask_loader=None, clip=False):
        """extracting.py:54-72 -> (mesh, stats_dict)."""
        if hasattr(self.model, 'eval'):
            self.model.eval()
        stats_dict = {}
        mesh = self.generate_from_latent(None, stats_dict=stats_dict, data=None, mask_loader=mask_loader, clip=clip)
        return mesh, stats_dict

    def generate_from_latent(self, c=None, stats_dict=None, data=None, mask_loader=None, **kwargs):
        """extracting.py:75-135."""
        stats_dict = {} if stats_dict is None else stats_dict
        if self.refinement_step > 0:
            raise NotImplementedError('Extractor3D: refinement_step > 0 (RMSprop refinement of the vertices, reference '
                                      'extracting.py:237-323) is not wired into generate_mesh; every shipped config uses 0.  Call '
                                      'Extractor3D.refine_mesh(mesh, steps=N) on the extracted mesh, or tools/refine_mesh.py on the file')
        if mask_loader is not None:
            raise NotImplementedError('Extractor3D: mask_loader (carving by dilated image masks, reference extracting.py:120-127, '
                                      '326-377) is not implemented: its projection assumes world -> NDC matrices, the data '
                                      'loader supplies camera-to-world poses and a pixel-unit K.  The same rule with this project\'s '
                                      'projection: Extractor3D(..., carve=psnerf_amd.hull.VisualHull.from_loader(mask_loader))')
        kwargs.setdefault('clip', False)
        threshold = iso_value(self.threshold)
        box_size = 2 + self.padding
        on_device = self.device.type == 'cuda'
        t0 = time.time()
        self.last_known = None
        if self.upsampling_steps == 0:                                             # extracting.py:90-96
            nx = self.resolution0
            pointsf = box_size * _make_3d_grid(nx)
            values = self.eval_points(pointsf.to(self.device), c, **kwargs)
            value_grid = values.reshape(nx, nx, nx).to(torch.float32)
            value_grid = value_grid.contiguous() if on_device else value_grid.cpu().numpy()
            stats_dict['n_points_evaluated'], stats_dict['n_rounds'] = nx ** 3, 1
        elif on_device:
            value_grid = self._mise_device(threshold, box_size, stats_dict, **kwargs)
        else:
            value_grid = self._mise_host(threshold, box_size, stats_dict, **kwargs)
        if on_device:
            torch.cuda.synchronize(self.device)
        stats_dict['time (eval points)'] = time.time() - t0
        if self.carve is not None:                                                 # extracting.py:120-127 (and hull.py on the projection)
            t1 = time.time()
            n = value_grid.shape[0]
            with Phase(self.phase_events, 'carve'):
                stats_dict['n_points_carved'] = self.carve.carve_grid(value_grid, box_size * torch.linspace(-0.5, 0.5, n))
            stats_dict['time (carve)'] = time.time() - t1
        if kwargs['clip']:                                                         # extracting.py:130-132
            n = value_grid.shape[0]
            z = box_size * torch.linspace(-0.5, 0.5, n)                            # the z coordinate of make_3d_grid
            below = z < -1
            if on_device:
                value_grid[:, :, below.to(self.device)] = -30.0
            else:
                value_grid[:, :, below.numpy()] = -30.0
        self.last_grid = value_grid
        return self.extract_mesh(value_grid, c, stats_dict=stats_dict)

    def eval_points(self, p, c=None, **kwargs):
        """extracting.py:137-155: the model's negated logits at p [Q, 3], in batches; returned on p's device."""
        outs = []
        pack = self._lean_pack() if self.device.type == 'cuda' else None
        for pi in torch.split(p, self.points_batch_size):
            if pack is not None:   # the lean engine on the batch (no scatter: the caller wants the values in order)
                outs.append(pack.on_points(pi.to(self.device).contiguous(), self.model.octaves_pe, 1.0 / self.model.rescale).reshape(-1))
                continue
            with torch.no_grad():
                occ_hat = self.model(pi.unsqueeze(0).to(self.device), None, return_logits=True, **kwargs).squeeze(-1)
            outs.append(occ_hat.squeeze(0).detach())
        return torch.cat(outs, dim=0) if outs else torch.zeros(0, device=self.device)

    def extract_mesh(self, occ_hat, c=None, stats_dict=None):
        """extracting.py:157-206: marching cubes on the padded grid, vertices to world units, optional normals."""
        stats_dict = {} if stats_dict is None else stats_dict
        box_size = 2 + self.padding
        threshold = iso_value(self.threshold)
        n = occ_hat.shape[0]
        assert tuple(occ_hat.shape) == (n, n, n), 'cubic value grids only'
        clean = self.keep_components is not None or self.min_component_faces > 0
        t0 = time.time()
        if torch.is_tensor(occ_hat) and occ_hat.is_cuda:
            from .. import hip
            with Phase(self.phase_events, 'marching cubes'):
                v, f = hip.marching_cubes(occ_hat.contiguous(), threshold, box_size)
            if clean:   # on the device tensors: less is copied back, fewer normals are computed
                from .. import meshclean
                torch.cuda.synchronize(occ_hat.device)
                t1 = time.time()
                with Phase(self.phase_events, 'components'):
                    v, f, _, report = meshclean._device_clean(v, f, None, self.keep_components, self.min_component_faces, 'faces')
                torch.cuda.synchronize(occ_hat.device)
                t0 += self._clean_stats(stats_dict, report, time.time() - t1)   # ('time (marching cubes)' stays what it was)
            if self.smooth_iterations is not None:   # on the device tensors, between the clean-up and the simplification
                from .. import meshsmooth
                torch.cuda.synchronize(occ_hat.device)
                t1 = time.time()
                with Phase(self.phase_events, 'smooth'):
                    v, report = meshsmooth._device_smooth(v, f, self.smooth_iterations, self.smooth_lambda, self.smooth_mu)
                torch.cuda.synchronize(occ_hat.device)
                t0 += self._smooth_stats(stats_dict, report, time.time() - t1)
            if self.simplify_nfaces is not None:   # likewise on the device tensors, after the clean-up
                from .. import meshsimplify
                torch.cuda.synchronize(occ_hat.device)
                t1 = time.time()
                n_from = f.shape[0]
                with Phase(self.phase_events, 'simplify'):
                    v, f, report = meshsimplify._device_simplify(v, f, target_faces=self.simplify_nfaces)
                torch.cuda.synchronize(occ_hat.device)
                t0 += self._simplify_stats(stats_dict, report, n_from, time.time() - t1)
            with Phase(self.phase_events, 'copy-back'):
                vertices, faces = v.cpu().numpy(), f.cpu().numpy()
            stats_dict['time (marching cubes)'] = time.time() - t0
        else:
            grid = occ_hat.numpy() if torch.is_tensor(occ_hat) else np.asarray(occ_hat)
            vertices, faces = host_marching_cubes(grid, threshold)
            vertices = to_world(vertices, n, box_size)
            stats_dict['time (marching cubes)'] = time.time() - t0
            if clean:
                from .. import meshclean
                t1 = time.time()
                vertices, faces, _, report = meshclean.host_clean(vertices, faces, None, self.keep_components, self.min_component_faces)
                self._clean_stats(stats_dict, report, time.time() - t1)
            if self.smooth_iterations is not None:
                from .. import meshsmooth
                t1 = time.time()
                vertices, report = meshsmooth.host_smooth(vertices, faces, self.smooth_iterations, self.smooth_lambda, self.smooth_mu)
                self._smooth_stats(stats_dict, report, time.time() - t1)
            if self.simplify_nfaces is not None:
                from .. import meshsimplify
                t1 = time.time()
                n_from = faces.shape[0]
                vertices, faces, report = meshsimplify.host_simplify(vertices, faces, target_faces=self.simplify_nfaces)
                self._simplify_stats(stats_dict, report, n_from, time.time() - t1)
        normals = None
        if self.with_normals and vertices.shape[0] != 0:
            t0 = time.time()
            normals = self.estimate_normals(vertices, c)
            stats_dict['time (normals)'] = time.time() - t0
        return Mesh(vertices, faces, vertex_normals=normals)

    @staticmethod
    def _clean_stats(stats_dict, report, seconds):
        stats_dict['n_components'], stats_dict['n_faces_removed'] = report['n_components'], report['n_faces_removed']
        stats_dict['time (components)'] = seconds
        return seconds

    @staticmethod
    def _simplify_stats(stats_dict, report, n_faces_from, seconds):
        stats_dict['n_faces_simplified_from'], stats_dict['simplify_resolution'] = int(n_faces_from), report['resolution']
        stats_dict['time (simplify)'] = seconds
        return seconds

    @staticmethod
    def _smooth_stats(stats_dict, report, seconds):
        stats_dict['smooth_iterations'], stats_dict['n_vertices_pinned'] = report['iterations'], report['n_pinned']
        stats_dict['smooth_max_displacement'], stats_dict['smooth_volume_ratio'] = report['max_displacement'], (
            report['volume_after'] / report['volume_before'] if report['volume_before'] != 0.0 else float('nan'))
        stats_dict['time (smooth)'] = seconds
        return seconds

    def estimate_normals(self, vertices, c=None):
        """extracting.py:209-235: -grad occupancy-logit / |.| at the vertices, through the model's ``gradient``."""
        normals = []
        for vi in torch.split(torch.as_tensor(np.asarray(vertices), dtype=torch.float32), self.points_batch_size):
            g = self.model.gradient(vi.unsqueeze(0).to(self.device), tflag=False).reshape(-1, 3)
            ni = -g
            ni = ni / torch.norm(ni, dim=-1, keepdim=True)
            normals.append(ni.cpu().numpy())
        return np.concatenate(normals, axis=0)

    def refine_mesh(self, mesh, occ_hat=None, c=None, steps=None, rng=None):
        """extracting.py:237-323: ``steps`` (default: self.refinement_step) RMSprop steps on the vertices -> a new Mesh with the same
        faces and vertex normals (the reference, too, estimates the normals before it refines).  ``occ_hat`` and ``c`` are accepted
        and unused, as in the reference (which only asserts the grid is cubic).  ``rng``: np.random-like (permutation, dirichlet),
        default the global np.random -- the reference shuffles with torch's DataLoader, so the face order is the same distribution
        but not bit-pinned to it.  An empty mesh, or steps <= 0, returns ``mesh`` itself.  Leaves
        self.last_refine = {'n_steps', 'time (refine)', 'loss_first', 'loss_last'}."""
        steps = self.refinement_step if steps is None else int(steps)
        if mesh.is_empty or len(mesh.faces) == 0 or steps <= 0:
            return mesh
        if hasattr(self.model, 'eval'):
            self.model.eval()
        t0 = time.time()
        v, losses = refine_vertices(self.model, mesh.vertices, mesh.faces, steps, self.refine_max_faces, self.threshold,
                                    np.random if rng is None else rng, self.device)
        self.last_refine = {'n_steps': len(losses), 'time (refine)': time.time() - t0, 'loss_first': losses[0], 'loss_last': losses[-1]}
        return Mesh(v.cpu().numpy().astype(np.float64), mesh.faces, vertex_normals=mesh.vertex_normals)

    # -- the two MISE drivers -------------------------------------------------------------------------------------------
    def _mise_host(self, threshold, box_size, stats_dict, **kwargs):
        mise = HostMISE(self.resolution0, self.upsampling_steps, threshold)
        n_eval = n_rounds = 0
        points = mise.query()
        while points.shape[0] != 0:                                                # extracting.py:101-116
            pointsf = grid_points_host(points, mise.resolution, box_size)
            values = self.eval_points(pointsf, None, **kwargs).cpu().numpy()
            mise.update(points, values)
            n_eval += points.shape[0]
            n_rounds += 1
            points = mise.query()
        stats_dict['n_points_evaluated'], stats_dict['n_rounds'] = n_eval, n_rounds
        self.last_known = mise.flags == 2
        return mise.to_dense()

    def _lean_pack(self):
        """The negated-logit pack of the lean engine if the model is a NeuralNetwork that engine holds, else None."""
        from .network import NeuralNetwork
        from .. import ops
        m = self.model
        if not isinstance(m, NeuralNetwork):
            return None
        if m._hidden_is_256() and m.d_pe <= 64 and m.lin0.weight_v.is_cuda:
            return m._logit_packed()
        ops.fallback('stage1 mesh extraction -> batched model calls', m.lin0.weight_v, 'hidden width is not 256')
        return None

    def _mise_device(self, threshold, box_size, stats_dict, **kwargs):
        from .. import hip
        dev = self.device
        res0, depth = int(self.resolution0), int(self.upsampling_steps)
        res = res0 << depth
        if res > hip.MESH_MAX_RESOLUTION:
            raise RuntimeError('Extractor3D: resolution %d > %d is not supported' % (res, hip.MESH_MAX_RESOLUTION))
        n = res + 1
        pack = self._lean_pack()
        grid = torch.full((n * n * n,), float('nan'), dtype=torch.float32, device=dev)
        flags = hip.mise_flags(res, dev)
        s = 1 << depth
        flags[:n * n * n].view(n, n, n)[::s, ::s, ::s] = 1
        vox = torch.zeros(sum((res0 << l) ** 3 for l in range(depth)), dtype=torch.uint8, device=dev)
        vox[:res0 ** 3] = 1
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        n_pending = (res0 + 1) ** 3
        n_eval = n_rounds = 0
        while n_pending > 0:
            with Phase(self.phase_events, 'collect + evaluate'):
                rows, points = hip.mise_collect(flags, res, box_size, n_pending, counts[0:1])
                if pack is not None:
                    pack.on_points(points, self.model.octaves_pe, 1.0 / self.model.rescale, out=grid, n_rows_dev=counts[0:1],
                                   out_rows=rows)
                else:
                    grid[rows] = self.eval_points(points, None, **kwargs).to(torch.float32)
            with Phase(self.phase_events, 'refine'):
                hip.mise_refine(grid, flags, vox, res0, depth, threshold, counts[1:2])
            n_eval += n_pending
            n_rounds += 1
            n_pending = int(counts[1].item())                                      # the round's only host synchronisation
        stats_dict['n_points_evaluated'], stats_dict['n_rounds'] = n_eval, n_rounds
        grid = grid.view(n, n, n)
        self.last_known = (flags[:n * n * n] == 2).view(n, n, n)
        with Phase(self.phase_events, 'fill'):
            hip.grid_ffill(grid)
        return grid


# ------------------------------------------------------------------------------------------------ vertex refinement
def _device_field(model, p):
    """(occupancy sigmoid(-10 logit) [F], -d occupancy / d p [F, 3]) of a device NeuralNetwork at p [F, 3], differentiable in p: one
    geometry-field call with its gradient sweep on DETACHED effective parameters (no parameter wants a gradient, so backward runs
    the two adjoint chains and csrc/geo_dp.hip and no weight-gradient launch); -d sigmoid(-10 l) / d p = 10 s (1 - s) d l / d p is
    formed with torch ops on the [F] / [F, 3] tensors."""
    with torch.no_grad():
        params = [t.detach() for t in model._geo_params()]
    chains = model._geo_chains(params) if model.USE_FUSED_CHAINS and model._geo_chains_fit() else None
    parts = [model._geo_call(q, True, params, chains) for q in torch.split(p, model.MAX_ROWS)]
    logit, grad = (torch.cat([q[i] for q in parts], 0) if len(parts) > 1 else parts[0][i] for i in (0, 2))
    occ = torch.sigmoid(logit[:, 0] * -10.0)
    return occ, (10.0 * occ * (1.0 - occ))[:, None] * grad


def refine_loss(model, v, faces, eps, threshold):
    """extracting.py:283-310 for vertices v [V, 3], a batch of faces [F, 3] (int64) and barycentric weights eps [F, 3]:
        face_point = sum(eps * v[faces]);  face_normal = cross(v1 - v0, v2 - v1) / (|.| + 1e-10)
        face_value = sigmoid(-10 logit(face_point));  normal_target = -d face_value.sum() / d face_point / (|.| + 1e-10)
        loss = mean((face_value - threshold)^2) + 0.01 mean(sum((face_normal - normal_target)^2))
    -> (loss, loss_target, loss_normal), differentiable in v.  ``model``: a psnerf_amd NeuralNetwork on the device (-> _device_field),
    or any callable with the reference's signature that autograd can differentiate twice (the reference's own form)."""
    from .network import NeuralNetwork
    face_vertex = v[faces]
    face_point = (face_vertex * eps[:, :, None]).sum(dim=1)
    face_v1 = face_vertex[:, 1, :] - face_vertex[:, 0, :]
    face_v2 = face_vertex[:, 2, :] - face_vertex[:, 1, :]
    face_normal = torch.cross(face_v1, face_v2, dim=1)
    face_normal = face_normal / (face_normal.norm(dim=1, keepdim=True) + 1e-10)
    if isinstance(model, NeuralNetwork):
        if not v.is_cuda:
            raise RuntimeError('refine_loss: psnerf_amd.stage1.NeuralNetwork runs on the device only; on the host use oracle.stage1.NeuralNetwork')
        face_value, normal_target = _device_field(model, face_point)
    else:
        face_value = torch.cat([model(p_split, None, only_occupancy=True).squeeze(-1)
                                for p_split in torch.split(face_point.unsqueeze(0), 20000, dim=1)], dim=1).squeeze(0)
        normal_target = -torch.autograd.grad([face_value.sum()], [face_point], create_graph=True)[0]
    normal_target = normal_target / (normal_target.norm(dim=1, keepdim=True) + 1e-10)
    loss_target = (face_value - threshold).pow(2).mean()
    loss_normal = (face_normal - normal_target).pow(2).sum(dim=1).mean()
    return loss_target + 0.01 * loss_normal, loss_target, loss_normal


def refine_vertices(model, vertices, faces, steps, max_faces, threshold, rng, device, dtype=torch.float32):
    """The loop of extracting.py:254-320: v = Parameter(vertices) in ``dtype`` on ``device``, RMSprop(lr = 1e-5), face batches of
    ``max_faces`` from a fresh rng.permutation per epoch, rng.dirichlet((0.5, 0.5, 0.5)) weights per step, exactly ``steps`` steps.
    -> (refined vertices [V, 3] detached, [loss of every step])"""
    v = torch.nn.Parameter(torch.as_tensor(np.asarray(vertices), dtype=dtype).to(device))
    faces = torch.as_tensor(np.asarray(faces), dtype=torch.long).to(device)
    optimizer = torch.optim.RMSprop([v], lr=1e-5)
    losses, it_r = [], 0
    while it_r < steps:
        perm = torch.as_tensor(np.asarray(rng.permutation(faces.shape[0])), dtype=torch.long)
        for f_idx in torch.split(perm, max_faces):
            f_it = faces[f_idx.to(device)]
            optimizer.zero_grad()
            eps = torch.as_tensor(rng.dirichlet((0.5, 0.5, 0.5), size=f_it.shape[0]), dtype=dtype).to(device)
            loss = refine_loss(model, v, f_it, eps, threshold)[0]
            loss.backward()
            optimizer.step()
            losses.append(loss.detach())
            it_r += 1
            if it_r >= steps:
                break
    return v.detach(), [float(l) for l in losses]


def _make_3d_grid(nx):
    """common.py make_3d_grid((-0.5,)*3, (0.5,)*3, (nx,)*3): [nx^3, 3], x-major."""
    ax = torch.linspace(-0.5, 0.5, nx)
    px = ax.view(-1, 1, 1).expand(nx, nx, nx).contiguous().view(-1)
    py = ax.view(1, -1, 1).expand(nx, nx, nx).contiguous().view(-1)
    pz = ax.view(1, 1, -1).expand(nx, nx, nx).contiguous().view(-1)
    return torch.stack([px, py, pz], dim=1)
