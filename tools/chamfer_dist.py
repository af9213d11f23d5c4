#!/usr/bin/env python
"""Chamfer distance between a predicted mesh and the ground-truth scan: the reference's chamfer_dist.py with its arguments.

    python tools/chamfer_dist.py --mesh_gt A.ply --mesh_pred B.obj [--num_samples 10000] [--seed S] [--no-cuda]
                                 [--keep-components K] [--align rigid|similarity]

prints ``Chamfer Distance (mm):  %.2f`` (value x 1000).  Meshes: .obj / .ply (psnerf_amd.meshdist.load_mesh).  On a GPU the meshes
are uploaded once and sampling and the distance queries run on the device (csrc/meshdist.hip); --no-cuda, or no GPU, takes the
numpy host path.  --keep-components K (not in the reference; off when absent) first reduces the PREDICTED mesh to its K largest
connected components by face count (psnerf_amd/meshclean.py), on the same path.  --seed makes the surface samples reproducible
(default: the global np.random, as the reference).  --align MODE (not in the reference; off when absent) first registers the PREDICTED
mesh to the ground truth by trimmed point-to-plane ICP (psnerf_amd/meshalign.py), on the same path, with samples drawn from a copy of
the generator's state; the line printed is then the Chamfer distance of the moved mesh."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Evaluation')
    parser.add_argument('--mesh_gt', type=str, required=True)
    parser.add_argument('--mesh_pred', type=str, required=True)
    parser.add_argument('--num_samples', type=int, default=10000)
    parser.add_argument('--seed', type=int, default=None)
    parser.add_argument('--no-cuda', action='store_true', help='Do not use cuda.')
    parser.add_argument('--keep-components', type=int, default=None, help='keep the K largest connected components of mesh_pred')
    parser.add_argument('--align', type=str, default=None, choices=('rigid', 'similarity'), help='register mesh_pred to mesh_gt first')
    args = parser.parse_args(argv)
    from psnerf_amd.meshdist import get_chamfer_dist, load_mesh
    mesh_gt = load_mesh(args.mesh_gt)
    mesh_pred = load_mesh(args.mesh_pred)
    is_cuda = torch.cuda.is_available() and not args.no_cuda
    if args.keep_components is not None:
        from psnerf_amd.meshclean import clean_mesh
        mesh_pred, report = clean_mesh(mesh_pred, keep=args.keep_components, device='cuda' if is_cuda else None)
        print('mesh_pred: %d of %d connected components kept, %d faces removed' % (report['n_kept'], report['n_components'],
                                                                                   report['n_faces_removed']))
    rng = np.random.RandomState(args.seed) if args.seed is not None else None
    if args.align is not None:
        from psnerf_amd import meshalign
        from psnerf_amd.mesheval import _rng_copy
        found = meshalign.align_mesh(mesh_pred, mesh_gt, mode=args.align, rng=_rng_copy(rng), device='cuda' if is_cuda else None)
        print('mesh_pred aligned (%s): scale %.9g, rms %.6g over %d rows, %d iterations, %s' % (
            args.align, found['scale'], found['rms'], found['used'], found['iterations'], 'converged' if found['converged'] else 'NOT converged'))
        mesh_pred = meshalign.apply(found['matrix'], mesh_pred)
    chamfer, _ = get_chamfer_dist(mesh_pred, mesh_gt, num_samples=args.num_samples, rng=rng, device='cuda' if is_cuda else None)
    print('Chamfer Distance (mm):  %.2f' % (chamfer * 1000))
    return chamfer


if __name__ == '__main__':
    main()
