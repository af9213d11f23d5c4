#!/usr/bin/env python
"""Refine the vertices of an extracted mesh against the trained stage-1 field: the RMSprop refinement of the reference's
Extractor3D.refine_mesh (stage1/model/extracting.py:237-323) as a tool of its own.

    python tools/refine_mesh.py --obj_name bear --expname test_1 [--exp_folder out] [--load_iter N]
                                --mesh IN.{obj,ply} --out OUT.{obj,ply} [--steps N] [--refine-max-faces F] [--seed S]

reads <exp_folder>/<obj_name>/<expname>/config.yaml and models/model[_N].pt like tools/extract_mesh.py, reads the mesh with
psnerf_amd.meshdist.load_mesh, runs N steps (default: the config's extraction.refinement_step) and writes the refined mesh.
On a GPU a step is one fused geometry-field call and its backward (psnerf_amd/stage1/extracting.py); --no-cuda evaluates the
field with the CPU oracle through autograd.  --seed seeds the face shuffle and the barycentric samples (numpy RandomState)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Refine the vertices of a mesh against the occupancy field.')
    parser.add_argument('--gpu', default=0, type=int, help='gpu')
    parser.add_argument('--no-cuda', action='store_true', help='Do not use cuda.')
    parser.add_argument('--obj_name', type=str, default='bunny')
    parser.add_argument('--expname', type=str, default='test_1')
    parser.add_argument('--exp_folder', type=str, default='out')
    parser.add_argument('--load_iter', type=int, default=None)
    parser.add_argument('--mesh', type=str, required=True, help='the mesh to refine (.obj / .ply)')
    parser.add_argument('--out', type=str, required=True, help='where the refined mesh is written (.obj / .ply)')
    parser.add_argument('--steps', type=int, default=-1, help='refinement steps (default: extraction.refinement_step of the config)')
    parser.add_argument('--refine-max-faces', type=int, default=10000, help='faces per step')
    parser.add_argument('--seed', type=int, default=0)
    args = parser.parse_args(argv)

    torch.manual_seed(0)
    from psnerf_amd import meshdist
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.stage1 import config
    from psnerf_amd.stage1.extracting import Extractor3D
    out_dir = os.path.join(args.exp_folder, args.obj_name, args.expname)
    cfg = config.load_config(os.path.join(out_dir, 'config.yaml'))
    is_cuda = torch.cuda.is_available() and not args.no_cuda
    device = torch.device('cuda:%d' % args.gpu if is_cuda else 'cpu')
    if is_cuda:
        from psnerf_amd.stage1 import NeuralNetwork
    else:
        from oracle.stage1 import NeuralNetwork  # the same state_dict keys, plain torch on the host
    model = NeuralNetwork(cfg)
    CheckpointIO(os.path.join(out_dir, 'models'), model=model).load('model_%d.pt' % args.load_iter if args.load_iter else 'model.pt')
    steps = args.steps if args.steps >= 0 else int(cfg['extraction'].get('refinement_step', 0))
    generator = Extractor3D(model, device=device, refine_max_faces=args.refine_max_faces)
    mesh = meshdist.load_mesh(args.mesh)
    refined = generator.refine_mesh(mesh, steps=steps, rng=np.random.RandomState(args.seed))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    refined.export(args.out)
    if refined is mesh:
        print('%s: %d vertices, %d faces, nothing to refine (0 steps or an empty mesh)' % (args.out, len(mesh.vertices), len(mesh.faces)))
    else:
        r = generator.last_refine
        print('%s: %d vertices, %d faces, %d steps in %.2f s, loss %.6g -> %.6g' % (
            args.out, len(refined.vertices), len(refined.faces), r['n_steps'], r['time (refine)'], r['loss_first'], r['loss_last']))
    return args.out


if __name__ == '__main__':
    main()
