#!/usr/bin/env python
"""Measure the view-projection kernel at the shipped extraction size and write profiles/mesh_project.json.

Mesh: the sphere-initialised BEAR network of tools/bench_mesh.py extracted at (resolution 64, upsampling_steps 3) and simplified to a
tenth of its faces (as tools/bench_occlusion.py does), its atlas rows at T = 2048; 20 views of 512 x 612 uint8 RGB on
synthetic.stage1_camera's intrinsics, poses by synthetic.look_at_pose on a ring around the object at two elevations.  The rows are
worked on in chunks of faces of about 2^20 rows, as meshbake.bake_views does, and the times of the chunks are summed.  HIP events on
the stream, --warmup warm-ups, then median / min / max of --repeats.
  * fused: psn_project_rows (meshproject.project_rows on prepared rows), with (row, view) pairs and candidate rays per second and,
    from the kernel's counter, ray-triangle tests per candidate ray;
  * materialised: the route there was before -- the four cheap tests in torch view by view, the surviving segments written out as
    origins and directions and handed to MeshIndex.ray_cast(any_hit=True) with sort=True and with sort=False, then the bilinear
    sampling and the weighted sums in torch (index_add); ``materialise``, ``ray_cast`` and ``sample`` are timed apart;
  * the whole meshbake.bake_views call.
The seen counts of the two routes are compared and recorded.  Nothing gates on these numbers.

    python tools/bench_project.py [--repeats 7] [--warmup 2] [--views 20] [--out profiles/mesh_project.json]
"""
import argparse
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import extracted_mesh, stat as _stat, write_profile  # noqa: E402
from bench_occlusion import add, timed  # noqa: E402


def candidates(p, n, views, H, W, bias):
    """The four cheap tests in torch, view by view -> (row int64 [P], view int64 [P], u [P], v [P], cosine [P], origins [P, 3],
    directions [P, 3]) of the surviving (row, view) pairs; torch's own arithmetic, so a pair on an edge may differ from the kernel's."""
    q = p + bias * n
    rows, vs, us, ws, cs, ds = [], [], [], [], [], []
    for k in range(views.shape[0]):
        t = views[k]
        Rm, o = t[0:9].reshape(3, 3), t[9:12]
        d = p - o
        x = (d[:, 0:1] * Rm[0] + d[:, 1:2] * Rm[1]) + d[:, 2:3] * Rm[2]
        pu, pv = t[13] + t[12] * (x[:, 0] / x[:, 2]), t[14] + t[12] * (x[:, 1] / x[:, 2])
        e = o - p
        c = (n * e).sum(dim=1) / e.norm(dim=1)
        keep = torch.nonzero((x[:, 2] > 0) & (pu >= 0) & (pu <= W - 1) & (pv >= 0) & (pv <= H - 1) & (c > 0)).reshape(-1)
        rows.append(keep)
        vs.append(torch.full_like(keep, k))
        us.append(pu[keep]); ws.append(pv[keep]); cs.append(c[keep]); ds.append(o - q[keep])
    rows = torch.cat(rows)
    return rows, torch.cat(vs), torch.cat(us), torch.cat(ws), torch.cat(cs), q[rows].contiguous(), torch.cat(ds).contiguous()


def sample(images, rows, view, pu, pv, c, seen, R):
    """The bilinear samples of the seen pairs and their weighted sums in torch -> (sum [R, C], sum_sq [R, C], weight [R], n_seen [R])."""
    H, W, C = images.shape[1:]
    rows, view, pu, pv, c = rows[seen], view[seen], pu[seen], pv[seen], c[seen]
    x0, y0 = pu.floor().long(), pv.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    fx, fy = (pu - x0)[:, None], (pv - y0)[:, None]
    px = lambda y, x: images[view, y, x].double() / 255.0
    val = (1.0 - fy) * ((1.0 - fx) * px(y0, x0) + fx * px(y0, x1)) + fy * ((1.0 - fx) * px(y1, x0) + fx * px(y1, x1))
    total = torch.zeros(R, C, dtype=torch.float64, device=images.device).index_add_(0, rows, c[:, None] * val)
    total_sq = torch.zeros(R, C, dtype=torch.float64, device=images.device).index_add_(0, rows, c[:, None] * (val * val))
    weight = torch.zeros(R, dtype=torch.float64, device=images.device).index_add_(0, rows, c)
    n_seen = torch.zeros(R, dtype=torch.int64, device=images.device).index_add_(0, rows, torch.ones_like(rows))
    return total, total_sq, weight, n_seen


def measure(v, f, T, images, K, poses, repeats, warmup, dev):
    from psnerf_amd import hull, meshbake as mb, meshdist as md, meshocclude as mo, meshproject as mp
    atlas = mb.Atlas(T, f.shape[0])
    index = md.MeshIndex(v, f)
    bias = mo.default_bias(index)
    views = torch.from_numpy(hull._views(K, poses)).to(dev)
    V, H, W, C = images.shape
    step = max(1, mb.CHUNK_ROWS // atlas.K)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    rows = atlas.F * atlas.K
    fused = mat = smp = None
    cast = {True: None, False: None}
    tests = {'fused': 0, True: 0, False: 0}
    seen = {'fused': 0, True: 0, False: 0}
    n_candidates = chunks = 0
    for f0 in range(0, atlas.F, step):
        f1 = min(f0 + step, atlas.F)
        p, _, n = mb.atlas_points(atlas, v, f, None, f0, f1)
        chunks += 1
        run = lambda **kw: index.project_rows(p, n, images, views, bias=bias, **kw)
        fused = add(fused, timed(run, warmup, repeats))
        counter.zero_()
        seen['fused'] += int(run(n_tests=counter).n_seen.sum())
        tests['fused'] += int(counter.item())
        mat = add(mat, timed(lambda: candidates(p, n, views, H, W, bias), warmup, repeats))
        row, view, pu, pv, c, o, d = candidates(p, n, views, H, W, bias)
        n_candidates += int(row.shape[0])
        for sort in (True, False):
            cast[sort] = add(cast[sort], timed(lambda: index.ray_cast(o, d, 0.0, 1.0, any_hit=True, sort=sort), warmup, repeats))
            counter.zero_()
            hit = index.ray_cast(o, d, 0.0, 1.0, any_hit=True, sort=sort, n_tests=counter)[3]
            tests[sort] += int(counter.item())
            seen[sort] += int((~hit).sum())
        smp = add(smp, timed(lambda: sample(images, row, view, pu, pv, c, ~hit, p.shape[0]), warmup, repeats))
        del row, view, pu, pv, c, o, d, hit
    whole = timed(lambda: mb.bake_views((v, f), images, K, poses, atlas=atlas), warmup, repeats)
    pairs = rows * V
    route = lambda sort: {'ray_cast_ms': cast[sort], 'route_median_ms': mat['median_ms'] + cast[sort]['median_ms'] + smp['median_ms'],
                          'triangle_tests_per_candidate_ray': tests[sort] / float(max(n_candidates, 1)), 'seen_pairs': seen[sort]}
    out = {'texture': T, 'faces': atlas.F, 'cell': atlas.c, 'rows': rows, 'views': V, 'image': [H, W, C], 'pairs': pairs, 'chunks': chunks, 'bias': bias,
           'candidate_rays': n_candidates, 'candidate_share': n_candidates / float(pairs), 'seen_share_of_candidates': seen['fused'] / float(max(n_candidates, 1)),
           'fused': {'kernel_ms': fused, 'pairs_per_s': pairs / (fused['median_ms'] * 1e-3), 'candidate_rays_per_s': n_candidates / (fused['median_ms'] * 1e-3),
                     'triangle_tests_per_candidate_ray': tests['fused'] / float(max(n_candidates, 1)), 'seen_pairs': seen['fused']},
           'materialise_ms': mat, 'sample_ms': smp, 'bytes_of_materialised_rays': 48 * n_candidates,
           'materialised_sorted': route(True), 'materialised_unsorted': route(False), 'bake_views_call_ms': whole,
           'mesh': {'cells': list(index.n), 'cell_edge': index.cell, 'list_entries': index.n_entries, 'oversize_list': index.n_over}}
    best = min(out['materialised_sorted']['route_median_ms'], out['materialised_unsorted']['route_median_ms'])
    out['fused_over_the_better_materialised_route'] = fused['median_ms'] / best
    return out


def cameras(n_views, cfg, H, W):
    from psnerf_amd.synthetic import look_at_pose, stage1_camera
    K = stage1_camera(cfg, h=H, w=W)[0][0].numpy()
    near, far = cfg['rendering']['near'], cfg['rendering']['far']
    poses = np.stack([look_at_pose(0.5 * (near + far), az_deg=360.0 * k / n_views, el_deg=(25.0, -10.0)[k % 2]).numpy() for k in range(n_views)])
    return K, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--views', type=int, default=20)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--upsampling-steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_project.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_project: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import meshsimplify, ops
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    cfg = stage1_cfg('bear')
    geo = s1.NeuralNetwork(cfg).to(dev)
    H, W = 512, 612
    K, poses = cameras(args.views, cfg, H, W)
    images = torch.randint(0, 256, (args.views, H, W, 3), dtype=torch.uint8, device=dev)
    out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'repeats': args.repeats, 'warmup': args.warmup,
           'grid': '%d^3' % ((args.resolution << args.upsampling_steps) + 1)}
    with ops.strict():
        v, f = extracted_mesh(geo, dev, args.resolution, args.upsampling_steps)
        sv, sf, _ = meshsimplify._device_simplify(v, f, target_faces=f.shape[0] // 10)
        out['a_tenth_of_the_faces_2048_V%d' % args.views] = measure(sv, sf, 2048, images, K, poses, args.repeats, args.warmup, dev)
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    out['note'] = ('HIP events on the stream; times are summed over the chunks of faces (about 2^20 rows each).  fused = psn_project_rows, thread '
                   'per row over all views, view table in LDS.  materialised = the cheap tests in torch view by view (materialise_ms), the '
                   'surviving segments written to memory and MeshIndex.ray_cast(any_hit=True) (ray_cast_ms; with sort=True it includes the sort '
                   'by entry cell), then bilinear sampling and index_add sums in torch (sample_ms).  seen_pairs of the two routes may differ on '
                   'pairs whose torch-formed test or segment differs in the last bit')
    write_profile(args.out, out)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
