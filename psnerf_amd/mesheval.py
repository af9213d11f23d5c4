"""Evaluation of a reconstructed mesh against a ground-truth scan: the table one reports next to the reference's Chamfer distance
(psnerf_amd.meshdist.get_chamfer_dist) -- accuracy / completeness, F-score at distance thresholds, normal consistency and volume
IoU.  The reference computes the Chamfer distance only.

One code path over ``MeshIndex`` (device tensors or ``device='cuda'``: csrc/meshdist.hip for the distances, csrc/meshinside.hip for
the inside test) and ``_HostMesh`` (numpy, the definition), as in get_chamfer_dist: every array below is a numpy array on the one
and a device tensor on the other, and only the reductions' results are read back.  All uniforms are drawn on the host from the
caller's ``np.random.RandomState``, so both paths consume the same stream: the surface samples of ``pred``, then of ``gt`` -- the
draws of get_chamfer_dist in its order --, then the IoU points.
"""
import numpy as np
import torch

from .meshcore import face_cross
from .meshdist import MeshIndex, _prepare

DEFAULT_THRESHOLDS = (0.005, 0.01, 0.02)   # fractions of the ground truth's bounding-box diagonal


def _xp(x):
    return torch if torch.is_tensor(x) else np


def _unit_face_normals(mesh):
    """Unit normals of a mesh's faces [F, 3]; the normal of a zero-area triangle is the zero vector."""
    xp = _xp(mesh.vertices)
    n = xp.stack(face_cross(mesh.vertices, mesh.faces), 1)
    length = xp.sqrt((n * n).sum(1))   # (a reduction: not the order of meshcore.face_areas' nx nx + ny ny + nz nz, and kept as it is)
    return n / xp.where(length > 0.0, length, xp.ones_like(length))[:, None]


def _box(mesh):
    if isinstance(mesh, MeshIndex):
        return np.asarray(mesh.lo, dtype=np.float64), np.asarray(mesh.hi, dtype=np.float64)   # (the exact minimum / maximum of the vertices)
    return mesh.vertices.min(axis=0), mesh.vertices.max(axis=0)


def _inside_open(mesh, points, vote):
    """-> (inside bool [N], open bool [N]) from the crossing counts: inside = the parity of ``above`` along axis 2 (with ``vote`` the
    majority of the three axes); open = the line along axis 2 crosses the mesh an odd number of times altogether."""
    inside, line_open = None, None
    for axis in ((2, 0, 1) if vote else (2,)):
        above, below, on = mesh.crossings(points, axis, below=True)
        if line_open is None:
            line_open = ((above + below + on) & 1) == 1
            inside = above & 1
        else:
            inside = inside + (above & 1)
    return inside >= (2 if vote else 1), line_open


def _rng_copy(rng):
    """A RandomState in the state of ``rng`` (None: of the global np.random), which itself is left untouched."""
    copy = np.random.RandomState()
    copy.set_state((np.random if rng is None else rng).get_state())
    return copy


def evaluate_mesh(pred, gt, num_samples=10000, thresholds=None, iou_points=100000, rng=None, device=None, vote=False, report=False,
                  align=None, align_options=None, visible_from=None):
    """Compare the mesh ``pred`` with the ground truth ``gt`` (anything with ``.vertices`` and ``.faces``) -> dict.  Device tensors, or
    ``device='cuda'``, take the device path; otherwise the numpy host path.  ``rng``: np.random.RandomState (default: the global
    np.random).

    Distances, over ``num_samples`` surface samples of each mesh (pred first, then gt: get_chamfer_dist's draws, so ``chamfer`` is
    that function's value bit for bit from an equal rng state):
      accuracy, completeness, chamfer        the mean distance pred -> gt, gt -> pred, and the mean of the two
      accuracy2, completeness2, chamfer2     the same on squared distances
    ``thresholds``: distances in mesh units; the default is 0.5 %, 1 % and 2 % of the diagonal of gt's bounding box.  Per threshold t
    (dicts keyed by the threshold as a float, in the caller's order; ``thresholds`` lists the keys):
      precision[t], recall[t]                the share of pred -> gt, gt -> pred distances <= t
      fscore[t]                              2 P R / (P + R), 0 when P + R = 0
      precision_count[t], recall_count[t]    the two integer counts
    Normals: normals_accuracy, normals_completeness and their mean ``normals`` = the mean of |n . n'| over the samples, n the unit
    normal of the face a sample was drawn from and n' that of the closest triangle of the other mesh; a zero-area triangle has the
    zero vector for a normal and contributes 0.
    Volume, over ``iou_points`` uniform points of the two meshes' joint bounding box (drawn after the surface samples and scaled
    into the box in float64 on the host; 0 skips the block), each tested against each mesh by the parity of its line's crossings
    (MeshIndex.crossings, axis 2; ``vote``: the majority of the three axes, for scans with holes):
      inside_pred, inside_gt, intersection, union   counts;  iou = intersection / union, NaN when the union is empty
      volume_pred, volume_gt                 count / iou_points x the box's volume
      open_pred, open_gt (n_open_*)          the share (count) of the points whose line along axis 2 crosses the mesh an odd number
                                             of times: 0 for a closed surface
    ``raw``: the samples, their faces, distances and closest triangles, and the IoU points with the two inside masks.
    ``report``: also pred_topology and gt_topology, the connectivity reports of the two meshes (meshtopo.mesh_report: edge classes,
    Euler characteristic, is_watertight, is_oriented, area, volume), which say WHY a line is not closed; nothing else changes.
    ``align``: None (default: the meshes are taken to be in one frame, and every output is what it was without the argument), or
    'rigid' / 'similarity': ``pred`` is first registered to ``gt`` (meshalign.align_mesh on the same path, with its defaults unless
    ``align_options``, a dict of its keyword arguments, says otherwise) and everything above is computed for the moved prediction;
    ``alignment`` then holds the registration's result without its history (matrix, scale, rotation, translation, rms, used,
    iterations, converged, mode).  The registration draws its samples from a COPY of the rng's state, so the evaluation's own draws
    are those of the call without ``align``.
    ``visible_from``: None (default: every output is what it was without the argument), or (camera_mats, world_mats, H, W): the
    samples are drawn exactly as without it, and each side's samples are then KEPT iff some view sees them on their OWN mesh
    (meshproject.project_rows without images or masks; the row normal is the sampled face's unit normal) -- a turntable rig never
    saw the underside, where the reconstruction is free invention and the scan is often open.  accuracy, completeness, their
    squared forms, chamfer, precision, recall, fscore, their counts and the normal consistency then run over the kept samples;
    ``visible_fraction_pred`` and ``visible_fraction_gt`` are the kept shares, raw['pred_visible'] / raw['gt_visible'] the masks (the
    other raw arrays keep all samples); the volume block is unchanged.  A side of which no sample is seen raises ValueError."""
    pred_m, gt_m = _prepare(pred, device, 'pred'), _prepare(gt, device, 'gt')
    alignment = None
    if align is not None:
        from . import meshalign
        if align not in ('rigid', 'similarity'):
            raise ValueError('evaluate_mesh: align=%r (None, \'rigid\' or \'similarity\')' % (align,))
        alignment = meshalign.align_mesh(pred_m, gt_m, mode=align, rng=_rng_copy(rng), **dict(align_options or {}))
        pred_m = meshalign.moved(pred_m, alignment['matrix'])
    pred_pts, pred_face = pred_m.sample_surface(num_samples, rng)
    gt_pts, gt_face = gt_m.sample_surface(num_samples, rng)
    _, pred_gt_dist, pred_gt_tri = gt_m.closest_point(pred_pts)
    _, gt_pred_dist, gt_pred_tri = pred_m.closest_point(gt_pts)
    out = {'num_samples': int(num_samples)}
    pred_n, gt_n = _unit_face_normals(pred_m), _unit_face_normals(gt_m)
    all_dist, all_tri, all_face = (pred_gt_dist, gt_pred_dist), (pred_gt_tri, gt_pred_tri), (pred_face, gt_face)
    visible = None
    if visible_from is not None:
        from . import meshproject
        camera_mats, world_mats, height, width = visible_from
        visible = []
        for side, m, pts, face, unit in (('pred', pred_m, pred_pts, pred_face, pred_n), ('gt', gt_m, gt_pts, gt_face, gt_n)):
            seen = meshproject.project_rows(m, pts, unit[face], None, camera_mats, world_mats, hw=(height, width)).n_seen > 0
            out['visible_fraction_' + side] = int(seen.sum()) / max(int(seen.shape[0]), 1)
            if out['visible_fraction_' + side] == 0.0:
                raise ValueError('evaluate_mesh: no sample of %s is seen by any view of visible_from' % side)
            visible.append(seen)
        pred_gt_dist, gt_pred_dist = pred_gt_dist[visible[0]], gt_pred_dist[visible[1]]
        pred_gt_tri, gt_pred_tri = pred_gt_tri[visible[0]], gt_pred_tri[visible[1]]
        pred_face, gt_face = pred_face[visible[0]], gt_face[visible[1]]
    out['chamfer'] = float((pred_gt_dist.mean() + gt_pred_dist.mean()) / 2)
    out['accuracy'], out['completeness'] = float(pred_gt_dist.mean()), float(gt_pred_dist.mean())
    out['accuracy2'], out['completeness2'] = float((pred_gt_dist * pred_gt_dist).mean()), float((gt_pred_dist * gt_pred_dist).mean())
    out['chamfer2'] = (out['accuracy2'] + out['completeness2']) / 2
    gt_lo, gt_hi = _box(gt_m)
    if thresholds is None:
        diagonal = float(np.sqrt(((gt_hi - gt_lo) ** 2).sum()))
        thresholds = [x * diagonal for x in DEFAULT_THRESHOLDS]
    out['thresholds'] = [float(t) for t in thresholds]
    for key in ('precision', 'recall', 'fscore', 'precision_count', 'recall_count'):
        out[key] = {}
    for t in out['thresholds']:
        n_p, n_r = int((pred_gt_dist <= t).sum()), int((gt_pred_dist <= t).sum())
        p, r = n_p / max(len(pred_gt_dist), 1), n_r / max(len(gt_pred_dist), 1)
        out['precision_count'][t], out['recall_count'][t], out['precision'][t], out['recall'][t] = n_p, n_r, p, r
        out['fscore'][t] = 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0
    out['normals_accuracy'] = float(abs((pred_n[pred_face] * gt_n[pred_gt_tri]).sum(1)).mean())
    out['normals_completeness'] = float(abs((gt_n[gt_face] * pred_n[gt_pred_tri]).sum(1)).mean())
    out['normals'] = (out['normals_accuracy'] + out['normals_completeness']) / 2
    raw = {'pred_surf_pts': pred_pts, 'gt_surf_pts': gt_pts, 'pred_face': all_face[0], 'gt_face': all_face[1], 'pred_gt_dist': all_dist[0],
           'gt_pred_dist': all_dist[1], 'pred_gt_tri': all_tri[0], 'gt_pred_tri': all_tri[1]}
    if visible is not None:
        raw['pred_visible'], raw['gt_visible'] = visible
    n_iou = int(iou_points)
    out['iou_points'] = n_iou
    if n_iou > 0:
        pred_lo, pred_hi = _box(pred_m)
        lo, hi = np.minimum(pred_lo, gt_lo), np.maximum(pred_hi, gt_hi)
        points = lo + (np.random if rng is None else rng).random_sample((n_iou, 3)) * (hi - lo)
        if isinstance(pred_m, MeshIndex):
            points = torch.from_numpy(points).to(pred_m.vertices.device)
        in_pred, open_pred = _inside_open(pred_m, points, vote)
        in_gt, open_gt = _inside_open(gt_m, points, vote)
        volume = float(np.prod(hi - lo))
        out['inside_pred'], out['inside_gt'] = int(in_pred.sum()), int(in_gt.sum())
        out['intersection'], out['union'] = int((in_pred & in_gt).sum()), int((in_pred | in_gt).sum())
        out['iou'] = out['intersection'] / out['union'] if out['union'] > 0 else float('nan')
        out['volume_pred'], out['volume_gt'] = out['inside_pred'] / n_iou * volume, out['inside_gt'] / n_iou * volume
        out['n_open_pred'], out['n_open_gt'] = int(open_pred.sum()), int(open_gt.sum())
        out['open_pred'], out['open_gt'] = out['n_open_pred'] / n_iou, out['n_open_gt'] / n_iou
        raw.update({'iou_pts': points, 'inside_pred': in_pred, 'inside_gt': in_gt})
    out['raw'] = raw
    if alignment is not None:
        out['alignment'] = {k: v for k, v in alignment.items() if k != 'history'}
    if report:
        from . import meshtopo
        for key, m in (('pred_topology', pred_m), ('gt_topology', gt_m)):
            out[key] = meshtopo.mesh_report((m.vertices, m.faces))
    return out
