#!/usr/bin/env python
"""Measure the occlusion bake's kernel at the shipped extraction size and write profiles/mesh_occlusion.json.

Mesh: the sphere-initialised BEAR network of tools/bench_mesh.py extracted at (resolution 64, upsampling_steps 3) and simplified to a
tenth of its faces (as tools/bench_bake.py does), its atlas rows at T = 2048 with K = 64 directions; with --full also every face of
the mesh at T = 4096 with K = 16.  The rows are worked on in chunks of faces of about 2^20 rows, as meshbake.bake_occlusion does, and
the times of the chunks are summed.  HIP events on the stream, --warmup warm-ups, then median / min / max of --repeats.  Per size:
  * fused: psn_occlusion_rows (meshocclude.occlusion_rows on prepared rows), with rays per second and, from the kernel's counter,
    ray-triangle tests per ray;
  * materialised: the same rays written out as origins and directions in the [K, R] layout meshrender.mesh_light_visibility uses
    and handed to MeshIndex.ray_cast(any_hit=True), with sort=True and with sort=False -- the only route before the fused kernel;
    ``materialise`` (forming the rays with torch) and ``ray_cast`` (the call, with its sort by entry cell where there is one) are
    timed apart, and the counter is read for both orders;
  * the whole meshbake.bake_occlusion call.
The blocked counts of the two routes are compared (they must be equal) and recorded.  Nothing gates on these numbers.

    python tools/bench_occlusion.py [--repeats 7] [--warmup 2] [--full] [--out profiles/mesh_occlusion.json]
"""
import argparse
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import extracted_mesh, stat as _stat, write_profile  # noqa: E402


def timed(fn, warmup, repeats):
    """fn() bracketed by HIP events -> stat over the repeats."""
    ms = []
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return _stat(ms)


def add(a, b):
    return b if a is None else {k: a[k] + b[k] for k in a}


def materialise(p, n, table, bias):
    """The rays of rows (p, n) in the [K, R] layout -> (origins [K R, 3], directions [K R, 3]); torch's own arithmetic, so the rays may
    differ from the kernel's in the last bit.  The frame is meshocclude.frame in torch."""
    s = torch.where(n[:, 2] >= 0.0, 1.0, -1.0).to(n.dtype)
    a = -1.0 / (s + n[:, 2])
    q = n[:, 0] * n[:, 1] * a
    t = torch.stack([1.0 + s * n[:, 0] * n[:, 0] * a, s * q, -s * n[:, 0]], dim=1)
    b = torch.stack([q, s + n[:, 1] * n[:, 1] * a, -n[:, 1]], dim=1)
    d = table[:, None, 0:1] * t[None] + table[:, None, 1:2] * b[None] + table[:, None, 2:3] * n[None]     # [K, R, 3]
    o = (p + bias * n)[None].expand(table.shape[0], -1, -1)
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def measure(v, f, T, K, repeats, warmup, dev):
    from psnerf_amd import meshbake as mb, meshdist as md, meshocclude as mo
    atlas = mb.Atlas(T, f.shape[0])
    index = md.MeshIndex(v, f)
    table = torch.from_numpy(mo.hemisphere_table(K)).to(dev)
    bias = mo.default_bias(index)
    step = max(1, mb.CHUNK_ROWS // atlas.K)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    rows = atlas.F * atlas.K
    fused = mat = None
    cast = {True: None, False: None}
    tests = {'fused': 0, True: 0, False: 0}
    blocked = {'fused': 0, True: 0, False: 0}
    live = chunks = 0
    for f0 in range(0, atlas.F, step):
        f1 = min(f0 + step, atlas.F)
        p, _, n = mb.atlas_points(atlas, v, f, None, f0, f1)
        chunks += 1
        fused = add(fused, timed(lambda: mo.occlusion_rows(index, p, n, table, bias=bias), warmup, repeats))
        counter.zero_()
        hits = mo.occlusion_rows(index, p, n, table, bias=bias, n_tests=counter)[0]
        tests['fused'] += int(counter.item())
        ok = hits >= 0
        live += int(ok.sum())
        blocked['fused'] += int(hits[ok].sum())
        mat = add(mat, timed(lambda: materialise(p, n, table, bias), warmup, repeats))
        o, d = materialise(p, n, table, bias)
        dead = (~ok)[None].expand(K, -1).reshape(-1)
        for sort in (True, False):
            cast[sort] = add(cast[sort], timed(lambda: index.ray_cast(o, d, 0.0, float('inf'), any_hit=True, sort=sort), warmup, repeats))
            counter.zero_()
            hit = index.ray_cast(o, d, 0.0, float('inf'), any_hit=True, sort=sort, n_tests=counter)[3]
            tests[sort] += int(counter.item())
            blocked[sort] += int((hit & ~dead).sum())
        del o, d
    whole = timed(lambda: mb.bake_occlusion((v, f), atlas=atlas, K=K), warmup, repeats)
    rays = live * K
    route = lambda sort: {'ray_cast_ms': cast[sort], 'materialise_plus_ray_cast_median_ms': mat['median_ms'] + cast[sort]['median_ms'],
                          'rays_per_s': rays / ((mat['median_ms'] + cast[sort]['median_ms']) * 1e-3),
                          'triangle_tests_per_ray': tests[sort] / float(rays), 'blocked': blocked[sort]}
    out = {'texture': T, 'faces': atlas.F, 'cell': atlas.c, 'rows': rows, 'rows_that_cast': live, 'directions': K, 'rays': rays, 'chunks': chunks,
           'bias': bias, 'blocked_share': blocked['fused'] / float(max(rays, 1)),
           'fused': {'kernel_ms': fused, 'rays_per_s': rays / (fused['median_ms'] * 1e-3), 'triangle_tests_per_ray': tests['fused'] / float(rays),
                     'blocked': blocked['fused']},
           'materialise_ms': mat, 'bytes_of_materialised_rays': 48 * rays,
           'materialised_sorted': route(True), 'materialised_unsorted': route(False),
           'bake_occlusion_call_ms': whole,
           'mesh': {'cells': list(index.n), 'cell_edge': index.cell, 'list_entries': index.n_entries, 'oversize_list': index.n_over}}
    best = min(out['materialised_sorted']['materialise_plus_ray_cast_median_ms'], out['materialised_unsorted']['materialise_plus_ray_cast_median_ms'])
    out['fused_over_the_better_materialised_route'] = fused['median_ms'] / best
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--upsampling-steps', type=int, default=3)
    ap.add_argument('--full', action='store_true', help='also every face of the mesh at T = 4096, K = 16')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_occlusion.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_occlusion: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import meshsimplify, ops
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    geo = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'repeats': args.repeats, 'warmup': args.warmup,
           'grid': '%d^3' % ((args.resolution << args.upsampling_steps) + 1)}
    with ops.strict():
        v, f = extracted_mesh(geo, dev, args.resolution, args.upsampling_steps)
        sv, sf, _ = meshsimplify._device_simplify(v, f, target_faces=f.shape[0] // 10)
        out['a_tenth_of_the_faces_2048_K64'] = measure(sv, sf, 2048, 64, args.repeats, args.warmup, dev)
        if args.full:
            out['full_mesh_4096_K16'] = measure(v, f, 4096, 16, args.repeats, args.warmup, dev)
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    out['note'] = ('HIP events on the stream; times are summed over the chunks of faces (about 2^20 rows each).  fused = psn_occlusion_rows, '
                   'thread per row, table in LDS.  materialised = origins and directions written to memory in the [K, R] layout, then '
                   'MeshIndex.ray_cast(any_hit=True): ray_cast_ms is that call (with sort=True it includes the sort by entry cell), '
                   'materialise_ms the forming of the rays with torch.  blocked = the rays that hit, over the rows that cast; the two routes '
                   'may differ on rays whose torch-formed direction differs in the last bit')
    write_profile(args.out, out)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
