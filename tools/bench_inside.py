#!/usr/bin/env python
"""Measure the inside test and the mesh evaluation at the shipped extraction size and write profiles/mesh_inside.json.

Mesh: the sphere-initialised BEAR network of tools/bench_mesh.py extracted at (resolution 64, upsampling_steps 3), kept on the
device, as the other mesh benches use it; the evaluation compares the (64, 2) extraction against it, as tools/bench_chamfer.py does.
HIP events around each workload, --warmup warm-ups, then median / min / max of --repeats:
  * 1 000 000 uniform points of the mesh's bounding box through psn_mesh_crossings: with and without ``below``, along axis 2 and
    axis 0, in sorted order (the sort outside the bracket) and as they come; MeshIndex.crossings and .contains as whole calls (the
    sort inside); line-triangle tests per point from the kernel's counter;
  * for context in the same run: MeshIndex.closest_point over the same points, and the numpy definition on 1 000 of them (reported as
    seconds per 1 000 points; its counts are compared with the device's);
  * one full evaluate_mesh at its defaults (10 000 samples, 100 000 IoU points) and at 1 000 000 / 1 000 000.
Nothing gates on these numbers.

    python tools/bench_inside.py [--repeats 7] [--warmup 2] [--out profiles/mesh_inside.json]
"""
import argparse
import os
import socket
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import extracted_mesh, write_profile  # noqa: E402
from tools.bench_raycast import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--host-points', type=int, default=1000, help='points given to the numpy definition')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_inside.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_inside: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import hip, meshdist as md, ops
    from psnerf_amd.mesheval import evaluate_mesh
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'repeats': args.repeats, 'warmup': args.warmup}
    with ops.strict():
        v, f = extracted_mesh(net, dev, 64, 3)
        coarse = extracted_mesh(net, dev, 64, 2)
        index = md.MeshIndex(v, f)
        lo, hi = np.asarray(index.lo), np.asarray(index.hi)
        n = args.points
        points = torch.from_numpy(lo + np.random.RandomState(0).random_sample((n, 3)) * (hi - lo)).to(dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        raw = lambda axis, order, below, n_tests=None: hip.mesh_crossings(index.index, points, axis=axis, order=order, want_below=below,
                                                                          want_on=below, n_tests=n_tests)
        kernel = {}
        for axis in (2, 0):
            order = index.home_order(points, ((axis + 1) % 3, (axis + 2) % 3, axis))
            for below in (True, False):
                key = 'axis %d, %s' % (axis, 'whole column (above, below, on)' if below else 'upward only (above)')
                row = {'sorted_ms': timed(lambda: raw(axis, order, below), args.warmup, args.repeats)[0],
                       'unsorted_ms': timed(lambda: raw(axis, None, below), args.warmup, args.repeats)[0]}
                counter.zero_()
                above = raw(axis, order, below, counter)[0]
                row['triangle_tests_per_point'] = counter.item() / float(n)
                row['points_per_s_sorted'] = n / (row['sorted_ms']['median_ms'] * 1e-3)
                row['inside'] = int((above & 1).sum())
                kernel[key] = row
        whole = {'crossings(points) axis 2': timed(lambda: index.crossings(points), args.warmup, args.repeats)[0],
                 'contains(points) axis 2': timed(lambda: index.contains(points), args.warmup, args.repeats)[0],
                 'contains(points, vote=True)': timed(lambda: index.contains(points, vote=True), args.warmup, args.repeats)[0],
                 'closest_point(points), for context': timed(lambda: index.closest_point(points), args.warmup, args.repeats)[0]}
        out['crossings'] = {'points': n, 'kernel': kernel, 'whole_call_ms': whole}

        # ---- the whole evaluation: (64, 2) against (64, 3)
        pred, gt = SimpleNamespace(vertices=coarse[0], faces=coarse[1]), SimpleNamespace(vertices=v, faces=f)
        evaluation = {}
        for name, samples, iou in (('defaults', 10000, 100000), ('1M samples, 1M IoU points', 1000000, 1000000)):
            stat, result = timed(lambda: evaluate_mesh(pred, gt, samples, iou_points=iou, rng=np.random.RandomState(0)), args.warmup, args.repeats)
            del result['raw']
            evaluation[name] = {'whole_call_ms': stat, 'result': result}
        out['evaluate_mesh'] = evaluation
    out['mesh'] = {'faces': int(index.faces.shape[0]), 'vertices': int(index.vertices.shape[0]), 'cells': list(index.n), 'cell_edge': index.cell,
                   'list_entries': index.n_entries, 'oversize_list': index.n_over, 'index_bytes': index.index_bytes,
                   'coarse_faces': int(coarse[1].shape[0])}

    # ---- the numpy definition on a sub-sample, for context
    pick = torch.linspace(0, n - 1, args.host_points, device=dev).long()
    dev_counts = [x[pick].cpu().numpy() for x in raw(2, None, True)]
    t0 = time.time()
    host_counts = md.host_crossings(index.vertices.cpu().numpy(), index.faces.cpu().numpy(), points[pick].cpu().numpy(), 2)
    out['numpy_definition'] = {'points': int(len(pick)), 'seconds_per_1000_points': (time.time() - t0) / len(pick) * 1000.0,
                               'counts_equal_to_the_device': bool(all(np.array_equal(a, b) for a, b in zip(host_counts, dev_counts)))}
    out['note'] = ('HIP events on the stream; "kernel" = psn_mesh_crossings alone on uploaded points, the sort outside the bracket; "whole_call" = '
                   'the public method, the sort by column inside; evaluate_mesh includes both index builds, the host draws and their upload')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
