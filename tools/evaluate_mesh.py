#!/usr/bin/env python
"""The evaluation table of a predicted mesh against the ground-truth scan: Chamfer distance, accuracy / completeness, F-score at
distance thresholds, normal consistency and volume IoU (psnerf_amd/mesheval.py).

    python tools/evaluate_mesh.py PRED GT [--samples 10000] [--thresholds T [T ...]] [--iou-points 100000] [--seed S] [--vote]
                                  [--device cuda|cpu] [--json] [--topology] [--align rigid|similarity] [--visible-from params.json]

Meshes: .obj / .ply (psnerf_amd.meshdist.load_mesh).  --thresholds are distances in mesh units (default: 0.5 %, 1 % and 2 % of the
diagonal of GT's bounding box).  --iou-points 0 skips the volume block; --vote takes the majority of the three axes' inside tests,
for scans with holes.  On a GPU (--device cuda, the default where one is present) the meshes are uploaded once and sampling, the
distance queries and the inside tests run on the device; otherwise the numpy host path.  --seed makes the samples reproducible.
--json prints the result as one JSON object instead of the table.  --topology adds the connectivity report of each mesh
(psnerf_amd/meshtopo.py: boundary, non-manifold and inconsistently wound edges, Euler characteristic, area, signed volume), which says
why a line is not closed.  --align MODE (off when absent) first registers PRED to GT by trimmed point-to-plane ICP
(psnerf_amd/meshalign.py), for a prediction in another frame or unit, and adds the transform to the output.  --visible-from
params.json (the dataset's cameras, 'K', 'pose_c2w' and 'imhw', or --image-size H W) scores only the samples some camera sees on
their own mesh (psnerf_amd/meshproject.py) and adds the kept shares; the IoU is unchanged."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Mesh evaluation')
    parser.add_argument('pred', type=str)
    parser.add_argument('gt', type=str)
    parser.add_argument('--samples', type=int, default=10000)
    parser.add_argument('--thresholds', type=float, nargs='+', default=None)
    parser.add_argument('--iou-points', type=int, default=100000)
    parser.add_argument('--seed', type=int, default=None)
    parser.add_argument('--vote', action='store_true')
    parser.add_argument('--device', type=str, default=None, choices=('cuda', 'cpu'))
    parser.add_argument('--json', action='store_true')
    parser.add_argument('--topology', action='store_true')
    parser.add_argument('--align', type=str, default=None, choices=('rigid', 'similarity'))
    parser.add_argument('--visible-from', type=str, default=None, metavar='PARAMS_JSON')
    parser.add_argument('--image-size', type=int, nargs=2, default=None, metavar=('H', 'W'))
    args = parser.parse_args(argv)
    from psnerf_amd.meshdist import load_mesh
    from psnerf_amd.mesheval import evaluate_mesh
    device = args.device if args.device is not None else ('cuda' if torch.cuda.is_available() else 'cpu')
    rng = np.random.RandomState(args.seed) if args.seed is not None else None
    visible_from = None
    if args.visible_from is not None:
        from psnerf_amd.hull import cameras_from_params
        K, poses, _, hw = cameras_from_params(args.visible_from)
        hw = tuple(args.image_size) if args.image_size is not None else hw
        if hw is None:
            parser.error('--visible-from: %s has no imhw; give --image-size H W' % args.visible_from)
        visible_from = (K, poses, hw[0], hw[1])
    result = evaluate_mesh(load_mesh(args.pred), load_mesh(args.gt), num_samples=args.samples, thresholds=args.thresholds,
                           iou_points=args.iou_points, rng=rng, device='cuda' if device == 'cuda' else None, vote=args.vote,
                           report=args.topology, align=args.align, visible_from=visible_from)
    del result['raw']
    if 'alignment' in result:
        result['alignment'] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in result['alignment'].items()}
    if args.json:
        print(json.dumps(result))
        return result
    if 'alignment' in result:
        a = result['alignment']
        print('Aligned (%s)%s scale %.9g, rms %.6g over %d rows, %d iterations, %s' % (a['mode'], ' ' * (9 - len(a['mode'])), a['scale'], a['rms'],
              a['used'], a['iterations'], 'converged' if a['converged'] else 'NOT converged'))
    print('Chamfer distance   %.6g   (accuracy %.6g, completeness %.6g)' % (result['chamfer'], result['accuracy'], result['completeness']))
    print('squared            %.6g   (accuracy %.6g, completeness %.6g)' % (result['chamfer2'], result['accuracy2'], result['completeness2']))
    for t in result['thresholds']:
        print('F-score @ %-8.4g %.4f     (precision %.4f, recall %.4f)' % (t, result['fscore'][t], result['precision'][t], result['recall'][t]))
    print('Normal consistency %.4f     (accuracy %.4f, completeness %.4f)' % (result['normals'], result['normals_accuracy'],
                                                                              result['normals_completeness']))
    if visible_from is not None:
        print('Seen by a camera   pred %.2f %%, gt %.2f %% of the samples (the lines above run over these)' % (
            100.0 * result['visible_fraction_pred'], 100.0 * result['visible_fraction_gt']))
    if result['iou_points'] > 0:
        print('Volume IoU         %.4f     (volume pred %.6g, gt %.6g; lines not closed: pred %.2f %%, gt %.2f %%)' % (
            result['iou'], result['volume_pred'], result['volume_gt'], 100.0 * result['open_pred'], 100.0 * result['open_gt']))
    if args.topology:
        from psnerf_amd.meshtopo import report_line
        for name in ('pred', 'gt'):
            print('%-4s topology      %s' % (name, report_line(result[name + '_topology'])))
    return result


if __name__ == '__main__':
    main()
