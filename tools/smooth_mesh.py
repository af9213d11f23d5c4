#!/usr/bin/env python
"""Smooth a mesh file with Taubin's lambda | mu filter (psnerf_amd/meshsmooth.py), which removes the marching-cubes staircase without
shrinking the object, or with the plain Laplacian.

    python tools/smooth_mesh.py IN OUT [--smooth N] [--smooth-lambda 0.5] [--smooth-mu -0.53] [--laplacian] [--no-pin]
                                       [--normals area|uniform] [--report] [--device cuda]

IN / OUT: .obj / .ply (psnerf_amd.meshdist.load_mesh, Mesh.export).  --smooth N: N pairs of steps (default 10); --laplacian: N plain
Laplacian steps with --smooth-lambda instead.  Vertices on the rim and on non-manifold edges are held unless --no-pin is given.
Incoming normals are not written: positions move; --normals forms new ones on the smoothed mesh.  --report prints the topology
before and after (psnerf_amd/meshtopo.py).  --device cuda runs on the device (csrc/meshtopo.hip); the default is the numpy definition
on the host."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Smooth a mesh with the lambda | mu filter.')
    parser.add_argument('mesh_in')
    parser.add_argument('mesh_out')
    parser.add_argument('--smooth', type=int, default=10, help='pairs of steps (plain steps with --laplacian)')
    parser.add_argument('--smooth-lambda', type=float, default=0.5, help='the shrinking factor, in (0, 1]')
    parser.add_argument('--smooth-mu', type=float, default=-0.53, help='the inflating factor, below -lambda')
    parser.add_argument('--laplacian', action='store_true', help='plain Laplacian steps: no inflating step')
    parser.add_argument('--no-pin', action='store_true', help='do not hold the rim and the non-manifold seams')
    parser.add_argument('--normals', type=str, default=None, choices=('area', 'uniform'), help='write vertex normals of the smoothed mesh')
    parser.add_argument('--report', action='store_true', help='print the topology before and after')
    parser.add_argument('--device', type=str, default=None, help="'cuda' for the device path")
    args = parser.parse_args(argv)
    from psnerf_amd.meshdist import load_mesh
    from psnerf_amd.meshsmooth import smooth_mesh
    from psnerf_amd.meshtopo import mesh_report, report_line
    mesh = load_mesh(args.mesh_in)
    if args.report:
        print('before: %s' % report_line(mesh_report((mesh.vertices, mesh.faces), device=args.device)))
    out, report = smooth_mesh((mesh.vertices, mesh.faces), iterations=args.smooth, lam=args.smooth_lambda,
                              mu=None if args.laplacian else args.smooth_mu, pin=None if args.no_pin else 'boundary', normals=args.normals,
                              device=args.device)
    out.export(args.mesh_out)
    ratio = report['volume_after'] / report['volume_before'] if report['volume_before'] != 0.0 else float('nan')
    print('%s: %d %s, %d vertices pinned, %d isolated, displacement max %.6g mean %.6g, area %.6g -> %.6g, volume %.6g -> %.6g (x %.4f)' % (
        args.mesh_out, report['iterations'], 'Laplacian steps' if args.laplacian else 'lambda | mu pairs', report['n_pinned'],
        report['n_isolated'], report['max_displacement'], report['mean_displacement'], report['area_before'], report['area_after'],
        report['volume_before'], report['volume_after'], ratio))
    if args.report:
        print('after:  %s' % report_line(mesh_report((out.vertices, out.faces), device=args.device)))
    return args.mesh_out, report


if __name__ == '__main__':
    main()
