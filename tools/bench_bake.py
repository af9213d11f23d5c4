#!/usr/bin/env python
"""Measure the material bake (psnerf_amd/meshbake.py, csrc/meshbake.hip) and write profiles/mesh_bake.json.

The mesh is the one of the shipped extraction setting (resolution 64, upsampling_steps 3 -> a 513^3 grid) of a sphere-initialised
stage-1 network, as tools/bench_mesh.py builds it; the materials are those of a ``bear_conf()`` PSNetwork (albedo and normal networks
4 x 128, SG-weight network 2 x 64 with 27 outputs).  Three sizes: every face of the mesh at T = 4096, and the mesh simplified to a
tenth of its faces (meshsimplify) at T = 2048 and at T = 4096.  Per size, HIP events on the stream, median / min / max of --repeats
after --warmup warm-ups:
  * the whole bake_materials call (wall time beside it) and its phases, summed over the chunks: points (psn_atlas_points), one phase
    per map (encoding + network + output glue) and scatter (psn_atlas_scatter / psn_atlas_fill and the allocation of the textures);
  * the brackets around the single C-ABI launches; texels per second; peak device memory.
Context, in the same run: the same three networks on as many CONTIGUOUS rows in one plain call each, and a device-to-device copy that
moves the bytes the two atlas kernels move (points: 60 B written per row; scatter: 4 C B read and 4 C B written per row, C = 33).

    python tools/bench_bake.py [--repeats 7] [--warmup 2] [--out profiles/mesh_bake.json]
"""
import argparse
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import extracted_mesh, stat as _stat, sum_kernels, sum_phases, write_profile  # noqa: E402


def timed(fn, warmup, repeats):
    out = []
    for it in range(warmup + repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1))
    return _stat(out)


def measure(net, v, f, T, repeats, warmup):
    from psnerf_amd import hip, meshbake as mb
    runs = []
    for it in range(warmup + repeats):
        mb.PHASE_EVENTS, hip.PROFILE_EVENTS = [], []
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.time()
        e0.record()
        baked = mb.bake_materials(net, (v, f), size=T)
        e1.record()
        torch.cuda.synchronize()
        wall = time.time() - t0
        phase, mb.PHASE_EVENTS = mb.PHASE_EVENTS, None
        kern, hip.PROFILE_EVENTS = hip.PROFILE_EVENTS, None
        peak = torch.cuda.max_memory_allocated() / 2.0 ** 20
        atlas = baked['atlas']
        del baked
        if it < warmup:
            continue
        runs.append(dict(phases=sum_phases(phase), kernels=sum_kernels(kern), call_ms=e0.elapsed_time(e1), wall_ms=1e3 * wall, peak_mib=peak))
    rows = atlas.F * atlas.K
    channels = 3 + net.nbasis + 3
    out = {'texture': T, 'faces': atlas.F, 'cell': atlas.c, 'rows_per_face': atlas.K, 'rows': rows, 'owned_fraction_of_the_texels': rows / float(T * T),
           'chunks': -(-atlas.F // max(1, mb.CHUNK_ROWS // atlas.K)), 'channels': channels,
           'call_ms': _stat([r['call_ms'] for r in runs]), 'wall_ms': _stat([r['wall_ms'] for r in runs]),
           'phases_ms': dict((k, _stat([r['phases'][k] for r in runs])) for k in sorted(runs[0]['phases'])),
           'kernel_launches_ms_summed_over_the_call': dict((k, _stat([r['kernels'][k] for r in runs])) for k in sorted(runs[0]['kernels'])),
           'peak_device_memory_mib': max(r['peak_mib'] for r in runs)}
    call = out['call_ms']['median_ms']
    out['texels_per_s'] = rows / (call * 1e-3)
    ph = out['phases_ms']
    out['atlas_kernels_ms'] = ph['points']['median_ms'] + ph['scatter']['median_ms']
    out['networks_ms'] = sum(ph[k]['median_ms'] for k in mb.MAPS)
    out['atlas_kernels_over_networks'] = out['atlas_kernels_ms'] / out['networks_ms']
    return out


def context(net, out, device, repeats, warmup):
    """Beside a measured size: the same networks on as many contiguous rows, one plain call each; a copy of the atlas kernels' bytes."""
    from psnerf_amd import meshbake as mb
    rows, channels = out['rows'], out['channels']
    x = (torch.rand(rows, 3, device=device) - 0.5) * 2.0
    nrm = torch.zeros(1, 3, dtype=torch.float64, device=device)
    plain = {}
    with torch.no_grad():
        for name in mb.MAPS:
            plain[name] = timed(lambda: mb.material_rows(net, x, nrm, (name,)), warmup, repeats)
    del x
    moved = rows * 60 + rows * channels * 8
    src = torch.empty(moved // 2, dtype=torch.uint8, device=device)
    dst = torch.empty_like(src)
    out['context'] = {'plain_networks_ms': plain, 'plain_networks_total_ms': sum(p['median_ms'] for p in plain.values()),
                      'bytes_moved_by_the_atlas_kernels': moved, 'device_to_device_copy_moving_those_bytes_ms': timed(lambda: dst.copy_(src), warmup, repeats)}
    out['context']['networks_chunked_over_plain'] = out['networks_ms'] / out['context']['plain_networks_total_ms']
    out['context']['atlas_kernels_over_copy'] = out['atlas_kernels_ms'] / out['context']['device_to_device_copy_moving_those_bytes_ms']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--upsampling-steps', type=int, default=3)
    ap.add_argument('--commit', default=None, help='the commit the tree stands on (default: git rev-parse, where there is a .git)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_bake.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_bake: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import meshsimplify, ops
    import psnerf_amd.stage1 as s1
    import psnerf_amd.stage2 as s2
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    geo = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    net = s2.PSNetwork(s2.bear_conf()).to(dev).eval()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            pass
    with ops.strict():
        v, f = extracted_mesh(geo, dev, args.resolution, args.upsampling_steps)
        sv, sf, report = meshsimplify._device_simplify(v, f, target_faces=f.shape[0] // 10)
        out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'parent_commit': commit,
               'grid': '%d^3' % ((args.resolution << args.upsampling_steps) + 1), 'repeats': args.repeats, 'warmup': args.warmup,
               'networks': 'bear_conf(): albedo 4 x 128 -> 3, SG weights 2 x 64 -> 27, normal 4 x 128 -> 3; 10 octaves',
               'a_tenth_of_the_faces_2048': measure(net, sv, sf, 2048, args.repeats, args.warmup),
               'a_tenth_of_the_faces_4096': measure(net, sv, sf, 4096, args.repeats, args.warmup),
               'full_mesh_4096': measure(net, v, f, 4096, args.repeats, args.warmup)}
        for key in ('a_tenth_of_the_faces_2048', 'a_tenth_of_the_faces_4096', 'full_mesh_4096'):      # (after every bake: the plain calls on all rows grow the engines' workspace)
            context(net, out[key], dev, args.repeats, args.warmup)
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    out['simplified_resolution'] = report['resolution']
    out['note'] = ('HIP events on the stream.  call = the whole bake_materials call on device tensors (index check, atlas, chunks); phases '
                   'partition the chunks\' device work: points, one phase per map (the first map of a chunk also encodes the points), '
                   'scatter (with the allocation and fill of the texture in the first chunk); kernel_launches = the brackets around single '
                   'C-ABI calls; context = the same networks on as many contiguous rows in one call each, and a copy that moves as many '
                   'bytes as psn_atlas_points writes and psn_atlas_scatter reads and writes; peak_device_memory = torch.cuda.max_memory_allocated over one '
                   'call, the mesh, both networks and the workspaces of earlier calls included')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
