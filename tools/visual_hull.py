#!/usr/bin/env python
"""The visual hull of a dataset's object masks as a mesh: what the silhouettes alone say about the shape.  Use it to check cameras and
masks before any training, or to get a bounding shape.

    python tools/visual_hull.py --cameras data/bear/params.json --masks data/bear/mask --resolution 256 --out hull.ply
                                [--radius 12] [--views 1 5 9] [--box-size 2.4] [--host]

--cameras is the dataset's params.json, read as tools/render_mesh.py reads it ('K', 'pose_c2w' in OpenGL axes, 'n_view'); --masks the
directory of view_VV.png.  The masks are dilated by disk(--radius) (12: what the reference's extractor uses; 0: the bare silhouettes).
A point of the (resolution + 1)^3 lattice of the box [-box-size / 2, box-size / 2]^3 belongs to the hull if some image contains it and
no image that contains it shows background there (psnerf_amd/hull.py); the mesh is marching cubes of that indicator, closed at the box.
Printed per view: how many lattice points that view was the FIRST to carve (views in ascending order).  A view with a wrong pose or
a wrong mask shows up there: it carves far more than its neighbours, or everything.
On a GPU everything runs on the device; --host takes the numpy definition."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description='The visual hull of a dataset\'s masks as a mesh.')
    ap.add_argument('--cameras', required=True, help='the dataset\'s params.json')
    ap.add_argument('--masks', required=True, help='directory of view_VV.png')
    ap.add_argument('--resolution', type=int, default=256, help='cells per axis')
    ap.add_argument('--out', required=True, help='.ply or .obj')
    ap.add_argument('--radius', type=int, default=12, help='radius of the disk the masks are dilated by')
    ap.add_argument('--views', type=int, nargs='*', default=None, help='view numbers from 1 (default: all)')
    ap.add_argument('--box-size', type=float, default=2.4, help='edge of the box (the extractor\'s 2 + padding)')
    ap.add_argument('--host', action='store_true', help='run the float64 numpy definition on the CPU')
    args = ap.parse_args(argv)

    import torch
    from psnerf_amd import hull
    if not args.host and not torch.cuda.is_available():
        raise SystemExit('visual_hull: no GPU visible (the device path has no fall-back; --host runs the numpy definition)')
    dev = None if args.host else torch.device('cuda:0')
    vh = hull.VisualHull.from_params(args.cameras, args.masks, views=args.views, footprint=hull.disk_footprint(args.radius), device=dev)
    n = args.resolution + 1
    axis = (args.box_size * torch.linspace(-0.5, 0.5, n)).numpy().astype(np.float64)
    n_views = vh.views.shape[0]
    tally = np.zeros(n_views + 2, dtype=np.int64)                 # carved_by + 2: unseen, kept, view 0, ...
    yz = np.stack([np.repeat(axis, n), np.tile(axis, n)], axis=1)
    for x in axis:                                                # one x slab of the lattice at a time
        slab = np.concatenate([np.full((n * n, 1), x), yz], axis=1)
        by = vh.carve_points(slab if dev is None else torch.from_numpy(slab).to(dev))[1]
        tally += np.bincount((by if dev is None else by.cpu().numpy()).astype(np.int64) + 2, minlength=n_views + 2)
    mesh = vh.mesh(args.resolution, args.box_size)
    mesh.export(args.out)
    numbers = args.views if args.views else list(range(1, n_views + 1))
    print('%s: %d vertices, %d faces; %d^3 lattice points: %d in the hull, %d in no image' % (
        args.out, len(mesh.vertices), len(mesh.faces), n, tally[1], tally[0]))
    for k, vi in enumerate(numbers):
        print('view_%02d: first to carve %d points (%.2f %%)' % (vi, tally[k + 2], 100.0 * tally[k + 2] / float(n ** 3)))
    return {'unseen': int(tally[0]), 'kept': int(tally[1]), 'views': [int(t) for t in tally[2:]]}


if __name__ == '__main__':
    main()
