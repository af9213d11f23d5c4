#!/usr/bin/env python
"""Extract the surface of a trained stage-1 model as a mesh: the reference's stage1/extract_mesh.py with its arguments.

    python tools/extract_mesh.py --obj_name bear --expname test_1 [--exp_folder out] [--test_out_dir test_out]
                                 [--load_iter N] [--upsampling-steps S] [--mesh_extension obj|ply] [--clip]
                                 [--keep-components K] [--min-component-faces N] [--simplify-nfaces N]
                                 [--smooth N [--smooth-lambda 0.5] [--smooth-mu -0.53]]
                                 [--carve-masks DIR --cameras params.json [--carve-radius 12] [--views 1 5 9]]

reads <exp_folder>/<obj_name>/<expname>/config.yaml and models/model[_N].pt, writes <test_out_dir>/<obj_name>/<expname>/mesh.<ext>.
On a GPU the whole extraction runs on the device (psnerf_amd/stage1/extracting.py); --no-cuda takes the numpy host path with the
model evaluated by the CPU oracle.  --keep-components K / --min-component-faces N (not in the reference; off when absent) keep the K
largest connected components of the mesh among those with at least N faces (psnerf_amd/meshclean.py): the floaters and inner shells
of a field trained from few views go before the mesh is written.  --simplify-nfaces N (off when absent) then reduces the mesh to at
most N faces by quadric vertex clustering (psnerf_amd/meshsimplify.py).  --smooth N (off when absent) runs N pairs of Taubin's
lambda | mu filter after the clean-up and before the simplification (psnerf_amd/meshsmooth.py): the lattice's staircase goes, the
volume stays; the rim of a clipped mesh is held.  --carve-masks DIR --cameras params.json (off when absent)
carve the dense value grid with the dataset's object masks DIR/view_VV.png before marching cubes (psnerf_amd/hull.py): a lattice point
that lies in no image, or that some image shows as background after its mask was dilated by disk(--carve-radius), is set to -30 --
the reference's mask_loader rule with this project's projection.  --views: the view numbers (from 1) to carve with (default: all)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Extract meshes from occupancy process.')
    parser.add_argument('--gpu', default=0, type=int, help='gpu')
    parser.add_argument('--no-cuda', action='store_true', help='Do not use cuda.')
    parser.add_argument('--upsampling-steps', type=int, default=-1, help='Overrites the default upsampling steps in config')
    parser.add_argument('--refinement-step', type=int, default=-1, help='Overrites the default refinement steps in config')
    parser.add_argument('--obj_name', type=str, default='bunny')
    parser.add_argument('--expname', type=str, default='test_1')
    parser.add_argument('--exp_folder', type=str, default='out')
    parser.add_argument('--test_out_dir', type=str, default='test_out')
    parser.add_argument('--load_iter', type=int, default=None)
    parser.add_argument('--mesh_extension', type=str, default='obj')
    parser.add_argument('--clip', action='store_true', default=False, help='clip the bottom area')
    parser.add_argument('--keep-components', type=int, default=None, help='keep the K largest connected components')
    parser.add_argument('--min-component-faces', type=int, default=0, help='drop connected components with fewer faces')
    parser.add_argument('--simplify-nfaces', type=int, default=None, help='simplify the mesh to at most this many faces')
    parser.add_argument('--smooth', type=int, default=None, help='pairs of Taubin smoothing steps, before the simplification')
    parser.add_argument('--smooth-lambda', type=float, default=0.5, help='the shrinking factor, in (0, 1]')
    parser.add_argument('--smooth-mu', type=float, default=-0.53, help='the inflating factor, below -lambda')
    parser.add_argument('--carve-masks', type=str, default=None, help='directory of view_VV.png object masks to carve the grid with')
    parser.add_argument('--cameras', type=str, default=None, help='the dataset\'s params.json (with --carve-masks)')
    parser.add_argument('--carve-radius', type=int, default=12, help='radius of the disk the masks are dilated by')
    parser.add_argument('--views', type=int, nargs='*', default=None, help='view numbers from 1 to carve with (default: all)')
    args = parser.parse_args(argv)
    if (args.carve_masks is None) != (args.cameras is None):
        parser.error('--carve-masks and --cameras go together')

    torch.manual_seed(0)
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.stage1 import config
    from psnerf_amd.stage1.extracting import Extractor3D
    out_dir = os.path.join(args.exp_folder, args.obj_name, args.expname)
    cfg = config.load_config(os.path.join(out_dir, 'config.yaml'))
    is_cuda = torch.cuda.is_available() and not args.no_cuda
    device = torch.device('cuda:%d' % args.gpu if is_cuda else 'cpu')
    if args.upsampling_steps != -1:
        cfg['extraction']['upsampling_steps'] = args.upsampling_steps
    if is_cuda:
        from psnerf_amd.stage1 import NeuralNetwork
    else:
        from oracle.stage1 import NeuralNetwork  # the same state_dict keys, plain torch on the host
    carve = None
    if args.carve_masks is not None:
        from psnerf_amd import hull
        carve = hull.VisualHull.from_params(args.cameras, args.carve_masks, views=args.views, footprint=hull.disk_footprint(args.carve_radius),
                                            device=device if is_cuda else None)
    model = NeuralNetwork(cfg)
    CheckpointIO(os.path.join(out_dir, 'models'), model=model).load('model_%d.pt' % args.load_iter if args.load_iter else 'model.pt')
    generator = Extractor3D(model, resolution0=cfg['extraction']['resolution'], upsampling_steps=cfg['extraction']['upsampling_steps'],
                            refinement_step=max(args.refinement_step, 0), device=device, keep_components=args.keep_components,
                            min_component_faces=args.min_component_faces, simplify_nfaces=args.simplify_nfaces, carve=carve,
                            smooth_iterations=args.smooth, smooth_lambda=args.smooth_lambda, smooth_mu=args.smooth_mu)
    model.eval()
    test_out_path = os.path.join(args.test_out_dir, args.obj_name, args.expname)
    os.makedirs(test_out_path, exist_ok=True)
    t0 = time.time()
    mesh, stats = generator.generate_mesh(mask_loader=None, clip=args.clip)
    mesh_out_file = os.path.join(test_out_path, 'mesh.%s' % args.mesh_extension)
    mesh.export(mesh_out_file)
    print('%s: %d vertices, %d faces, %d points evaluated in %d rounds, %.2f s' % (
        mesh_out_file, len(mesh.vertices), len(mesh.faces), stats['n_points_evaluated'], stats['n_rounds'], time.time() - t0))
    if 'n_points_carved' in stats:
        print('%d lattice points carved by the masks of %d views' % (stats['n_points_carved'], carve.views.shape[0]))
    if 'n_components' in stats:
        print('%d connected components, %d faces removed' % (stats['n_components'], stats['n_faces_removed']))
    if 'smooth_iterations' in stats:
        print('smoothed by %d lambda | mu pairs: %d vertices pinned, largest displacement %.6g, volume x %.4f' % (
            stats['smooth_iterations'], stats['n_vertices_pinned'], stats['smooth_max_displacement'], stats['smooth_volume_ratio']))
    if 'n_faces_simplified_from' in stats:
        print('simplified from %d faces (grid resolution %s)' % (stats['n_faces_simplified_from'], stats['simplify_resolution']))
    return mesh_out_file


if __name__ == '__main__':
    main()
