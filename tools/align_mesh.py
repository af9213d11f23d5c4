#!/usr/bin/env python
"""Register one mesh to another by trimmed point-to-plane ICP (psnerf_amd/meshalign.py): the step between exporting a mesh and
evaluating it against a scan that is in another frame or unit.

    python tools/align_mesh.py SRC TGT [--mode rigid|similarity|translation] [--out aligned.ply] [--matrix m.json] [--samples 20000]
                               [--keep 0.9] [--max-dist D] [--symmetric] [--starts axes24] [--init moments|none|M.json] [--seed S]
                               [--device cuda|cpu]

Meshes: .obj / .ply (psnerf_amd.meshdist.load_mesh).  Prints the scale, rotation and translation that take SRC to TGT, the RMS
distance of the kept rows and whether the iteration converged; --out writes SRC moved by it (.obj / .ply; vertex normals are rotated,
faces unchanged), --matrix the 4 x 4 matrix and the report as JSON.  --starts axes24 tries the 24 axis permutations first, for a scan
with another up axis.  --init: the start ('moments': centroids and area, the default; 'none': the identity; a JSON file holding a
4 x 4 matrix or an object with a 'matrix' entry, e.g. an earlier --matrix output).  On a GPU (--device cuda, the default where one is
present) the closest-point queries and the sums run on the device; otherwise the numpy host path, which is quadratic in the mesh
size.  --seed makes the samples reproducible."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Mesh registration')
    parser.add_argument('src', type=str)
    parser.add_argument('tgt', type=str)
    parser.add_argument('--mode', type=str, default='rigid', choices=('rigid', 'similarity', 'translation'))
    parser.add_argument('--out', type=str, default=None)
    parser.add_argument('--matrix', type=str, default=None)
    parser.add_argument('--samples', type=int, default=20000)
    parser.add_argument('--keep', type=float, default=0.9)
    parser.add_argument('--max-dist', type=float, default=None)
    parser.add_argument('--symmetric', action='store_true')
    parser.add_argument('--starts', type=str, default=None, choices=('axes24',))
    parser.add_argument('--init', type=str, default='moments')
    parser.add_argument('--max-iterations', type=int, default=50)
    parser.add_argument('--seed', type=int, default=None)
    parser.add_argument('--device', type=str, default=None, choices=('cuda', 'cpu'))
    args = parser.parse_args(argv)
    from psnerf_amd import meshalign
    from psnerf_amd.meshdist import load_mesh
    device = args.device if args.device is not None else ('cuda' if torch.cuda.is_available() else 'cpu')
    init = args.init
    if init == 'none':
        init = None
    elif init != 'moments':
        with open(init) as fh:
            loaded = json.load(fh)
        init = np.asarray(loaded['matrix'] if isinstance(loaded, dict) else loaded, dtype=np.float64)
    src, tgt = load_mesh(args.src), load_mesh(args.tgt)
    rng = np.random.RandomState(args.seed) if args.seed is not None else None
    result = meshalign.align_mesh(src, tgt, mode=args.mode, samples=args.samples, keep=args.keep, symmetric=args.symmetric,
                                  max_iterations=args.max_iterations, init=init, starts=args.starts, rng=rng,
                                  device='cuda' if device == 'cuda' else None, max_dist=args.max_dist)
    print('scale        %.12g' % result['scale'])
    for row in result['rotation']:
        print('rotation     % .12f % .12f % .12f' % tuple(row))
    print('translation  %.12g %.12g %.12g' % tuple(result['translation']))
    print('rms %.6g over %d used rows (max_dist %.6g), %d iterations, %s%s' % (
        result['rms'], result['used'], result['max_dist'], result['iterations'], 'converged' if result['converged'] else 'NOT converged',
        '' if result['start'] is None else ', start %d' % result['start']))
    if args.out is not None:
        meshalign.apply(result['matrix'], src).export(args.out)
        print('wrote', args.out)
    if args.matrix is not None:
        report = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in result.items() if k != 'history'}
        report['history'] = [{k: v for k, v in h.items() if k not in ('matrix', 'transform')} for h in result['history']]
        with open(args.matrix, 'w') as fh:
            json.dump(report, fh, indent=1)
            fh.write('\n')
        print('wrote', args.matrix)
    return result


if __name__ == '__main__':
    main()
