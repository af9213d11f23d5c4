#!/usr/bin/env python
"""Measure the device mesh registration (psnerf_amd/meshalign.py, csrc/meshalign.hip around MeshIndex.closest_point) and write
profiles/mesh_align.json, by the protocol of tools/bench_smooth.py: HIP-event time per phase, median of 7 after 2 warm-ups.

The pair: the mesh of the shipped extraction setting (resolution 64, upsampling_steps 3 -> a 513^3 grid) of a sphere-initialised
stage-1 network is the target, the (64, 2) extraction of the same network moved by a known similarity the source.  The network's
surface is a sphere to within the network's wobble, about which a rotation cannot be observed; so that the recovered transform can be
held against the known one, BOTH meshes are first deformed by the same smooth map without a symmetry (the tests' x (1 + 0.25 x +
0.15 y^2 - 0.2 x z + 0.1 z) (1, 0.8, 0.65), applied to the vertices normalised by the mean radius).  Sizes, and with them the
times, are those of the extractions.

Reported: per iteration (one align_step under a mid-run transform, 20 000 samples, plain and symmetric) the phases transform /
closest point / quantile (psn_align_dist, torch.kthvalue and its host read) / sums (psn_align_sums and the read of the 37 + 4
numbers) and the host solve; the bracketed kernel launches; the whole align_mesh call (wall clock, synchronised) with its iteration
count; and the recovered transform against the known one.  A record: there is no time gate.

    python tools/bench_align.py [--repeats 7] [--warmup 2] [--samples 20000] [--out profiles/mesh_align.json]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import extracted_mesh, stat as _stat, sum_kernels, sum_phases, write_profile  # noqa: E402


def deform(v):
    """The smooth map without a symmetry, on device vertices scaled to mean radius 1 about their centroid."""
    c = v.mean(dim=0)
    u = v - c
    u = u / u.norm(dim=1).mean()
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    w = u * (1.0 + 0.25 * x + 0.15 * y * y - 0.2 * x * z + 0.1 * z)[:, None]
    return (w * torch.tensor([1.0, 0.8, 0.65], dtype=v.dtype, device=v.device)).contiguous()


def errors(found, moved_by, diag):
    E = np.asarray(found) @ np.asarray(moved_by)
    s = np.linalg.det(E[:3, :3]) ** (1.0 / 3.0)
    R = E[:3, :3] / s
    sine = min(1.0, np.linalg.norm(R - R.T) / (2.0 * np.sqrt(2.0)))
    angle = np.degrees(np.arcsin(sine)) if np.trace(R) > 1.0 else 180.0 - np.degrees(np.arcsin(sine))
    return {'rotation_deg': float(angle), 'translation_over_diagonal': float(np.linalg.norm(E[:3, 3]) / diag), 'scale': float(abs(s - 1.0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--samples', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_align.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_align: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import hip, meshalign as ma, ops
    from psnerf_amd.meshdist import MeshIndex
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    known = np.eye(4)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    known[:3, :3] = 1.04 * ma.rodrigues(np.radians(8.0) * axis)
    with ops.strict():
        tv, tf = extracted_mesh(net, dev, 64, 3)
        sv, sf = extracted_mesh(net, dev, 64, 2)
        tv, sv = deform(tv.to(torch.float64)), deform(sv.to(torch.float64))
        tgt = MeshIndex(tv, tf)
        diag = ma._diag(tgt)
        known[:3, 3] = 0.03 * diag * np.array([0.6, 0.64, -0.48])
        src = MeshIndex(hip.align_transform(sv, *ma.from_matrix(known)), sf)
        out = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'warmup': args.warmup, 'samples': args.samples,
               'target': {'vertices': int(tv.shape[0]), 'faces': int(tf.shape[0]), 'grid': '513^3'},
               'source': {'vertices': int(sv.shape[0]), 'faces': int(sf.shape[0]), 'grid': '257^3'},
               'known': {'rotation_deg': 8.0, 'translation_over_diagonal': 0.03, 'scale': 1.04}, 'modes': {}}
        for name, symmetric in (('plain', False), ('symmetric', True)):
            torch.cuda.synchronize()
            t0 = time.time()
            whole = ma.align_mesh(src, tgt, mode='similarity', samples=args.samples, symmetric=symmetric, rng=np.random.RandomState(0))
            torch.cuda.synchronize()
            first_wall = 1e3 * (time.time() - t0)
            rng = np.random.RandomState(0)
            x = src.sample_surface(args.samples, rng)[0]
            y = tgt.sample_surface(args.samples, rng)[0] if symmetric else None
            mid = whole['history'][min(2, len(whole['history']) - 1)]['transform']
            runs, walls = [], []
            for it in range(args.warmup + args.repeats):
                events, hip.PROFILE_EVENTS = [], []
                torch.cuda.synchronize()
                step = ma.align_step(src, tgt, x, y, mid, keep=0.9, symmetric=symmetric, phases=events)
                torch.cuda.synchronize()
                t0 = time.time()
                ma.solve_update(step['sums'], 'similarity')
                solve_ms = 1e3 * (time.time() - t0)
                kern, hip.PROFILE_EVENTS = hip.PROFILE_EVENTS, None
                t0 = time.time()
                again = ma.align_mesh(src, tgt, mode='similarity', samples=args.samples, symmetric=symmetric, rng=np.random.RandomState(0))
                torch.cuda.synchronize()
                wall = 1e3 * (time.time() - t0)
                if it >= args.warmup:
                    runs.append(dict(phases=sum_phases(events), kernels=sum_kernels(kern), solve_ms=solve_ms))
                    walls.append(wall)
            out['modes'][name] = {
                'rows_per_iteration': int(step['counts'].sum()), 'used': step['used'],
                'iteration_phases_ms': dict((k, _stat([r['phases'][k] for r in runs])) for k in sorted(runs[0]['phases'])),
                'iteration_kernel_launches_ms': dict((k, _stat([r['kernels'][k] for r in runs])) for k in sorted(runs[0]['kernels'])),
                'host_solve_ms': _stat([r['solve_ms'] for r in runs]),
                'whole_call_wall_ms': _stat(walls), 'whole_call_first_wall_ms': first_wall,
                'iterations': whole['iterations'], 'converged': whole['converged'], 'rms_over_diagonal': whole['rms'] / diag,
                'same_result_every_call': bool(np.array_equal(again['matrix'], whole['matrix'])),
                'rms_per_iteration_over_diagonal': [h['rms'] / diag for h in whole['history']],
                'error_against_the_known_transform': errors(whole['matrix'], known, diag)}
    out['note'] = ('iteration_phases = HIP events on the stream around the steps of one align_step: "transform" (psn_align_transform), '
                   '"closest_point" (MeshIndex.closest_point with its sort by home cell), "quantile" (psn_align_dist, torch.kthvalue and the '
                   'host read of max_dist), "sums" (psn_align_sums and the host read of the 37 + 4 numbers); symmetric rows do each '
                   'twice (three transforms).  host_solve = the 7 x 7 np.linalg.solve, wall clock.  whole_call = align_mesh with its '
                   'moments start, sampling, every iteration and the last pass, wall clock around a synchronised call.  The two '
                   'meshes are different triangulations of one surface, so the residual at the optimum is their discretisation '
                   'difference, not zero, and the error against the known transform is bounded by it, not by rounding.')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
