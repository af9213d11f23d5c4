#!/usr/bin/env python
"""Simplify a mesh file by quadric vertex clustering (psnerf_amd/meshsimplify.py): to a face budget, a cell edge or a grid resolution.

    python tools/simplify_mesh.py IN OUT (--target-faces N | --cell H | --resolution N) [--regularisation R] [--device cuda]

IN / OUT: .obj / .ply (psnerf_amd.meshdist.load_mesh, Mesh.export).  --device cuda runs on the device (csrc/meshsimplify.hip); the
default is the numpy definition on the host.  Normals are not written: positions move."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Simplify a mesh by quadric vertex clustering.')
    parser.add_argument('mesh_in')
    parser.add_argument('mesh_out')
    size = parser.add_mutually_exclusive_group(required=True)
    size.add_argument('--target-faces', type=int, default=None, help='at most this many faces')
    size.add_argument('--cell', type=float, default=None, help='the edge of a grid cell')
    size.add_argument('--resolution', type=int, default=None, help='cells along the longest axis of the bounding box')
    parser.add_argument('--regularisation', type=float, default=1e-3)
    parser.add_argument('--device', type=str, default=None, help="'cuda' for the device path")
    args = parser.parse_args(argv)
    from psnerf_amd.meshdist import load_mesh
    from psnerf_amd.meshsimplify import simplify_mesh
    mesh = load_mesh(args.mesh_in)
    out, report = simplify_mesh((mesh.vertices, mesh.faces), target_faces=args.target_faces, cell=args.cell, resolution=args.resolution,
                                regularisation=args.regularisation, device=args.device)
    out.export(args.mesh_out)
    if report.get('unchanged'):
        print('%s: %d faces, within the budget: written unchanged' % (args.mesh_out, len(out.faces)))
    else:
        print('%s: %d -> %d vertices, %d -> %d faces (resolution %s, cell %.6g, %d clusters, %d degenerate, %d duplicate, %d flipped, %d clamped%s)' % (
            args.mesh_out, len(mesh.vertices), len(out.vertices), len(mesh.faces), len(out.faces), report['resolution'], report['cell'],
            report['n_clusters'], report['n_faces_degenerate'], report['n_faces_duplicate'], report['n_faces_flipped'], report['n_clamped'],
            ', target missed' if report.get('target_missed') else ''))
    return args.mesh_out, report


if __name__ == '__main__':
    main()
