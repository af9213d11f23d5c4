#!/usr/bin/env python
"""Chamfer distance between a predicted mesh and the ground-truth scan: the reference's chamfer_dist.py with its arguments.

    python tools/chamfer_dist.py --mesh_gt A.ply --mesh_pred B.obj [--num_samples 10000] [--seed S] [--no-cuda]
                                 [--keep-components K]

prints ``Chamfer Distance (mm):  %.2f`` (value x 1000).  Meshes: .obj / .ply (psnerf_amd.meshdist.load_mesh).  On a GPU the meshes
are uploaded once and sampling and the distance queries run on the device (csrc/meshdist.hip); --no-cuda, or no GPU, takes the
numpy host path.  --keep-components K (not in the reference; off when absent) first reduces the PREDICTED mesh to its K largest
connected components by face count (psnerf_amd/meshclean.py), on the same path.  --seed makes the surface samples reproducible
(default: the global np.random, as the reference)."""
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
    chamfer, _ = get_chamfer_dist(mesh_pred, mesh_gt, num_samples=args.num_samples, rng=rng, device='cuda' if is_cuda else None)
    print('Chamfer Distance (mm):  %.2f' % (chamfer * 1000))
    return chamfer


if __name__ == '__main__':
    main()
