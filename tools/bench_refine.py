#!/usr/bin/env python
"""Measure the point gradient of the stage-1 geometry field and the vertex refinement built on it, and write
profiles/mesh_refine.json (HIP events, median / min / max over the repeats):

  (a) psn_geo_point_grad at 10,000 and 262,144 rows (h0 = hs = 256, n_freqs = 6, with the second-order group) against the same
      result composed from the launches that existed before it: two hip.gemm into a [Q, 64] buffer, hip.pe_encode_bwd, and the
      second-derivative term in torch (hip.pe_encode for the sin / cos columns, five elementwise / reduction ops);
  (b) one refinement step at refine_max_faces = 10000 on the mesh of the shipped extraction setting (resolution 64,
      upsampling_steps 3) of a sphere-initialised network, split into field forward, field backward and the rest;
  (c) ops.GeoFieldFused forward + backward at 262,144 points with p requiring a gradient against the same call without.

    python tools/bench_refine.py [--repeats 7] [--warmup 2] [--out profiles/mesh_refine.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import stat as _stat  # noqa: E402


def _timed(fn, repeats, warmup, inner=1):
    """ms per call of fn(): ``inner`` back-to-back calls between two events, per repeat."""
    out = []
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) / inner)
    return _stat(out)


def bench_kernel(n, dev, repeats, warmup, n_freqs=6, h=256):
    from psnerf_amd import hip
    g = torch.Generator().manual_seed(n)
    d_pe = 3 + 6 * n_freqs
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    p, dz0, dzs, d_grad = (torch.rand(n, 3, generator=g) * 1.6 - 0.8).to(dev), r(n, h), r(n, h), r(n, 3)
    w0, ws = torch.zeros(h, 64, device=dev), torch.zeros(h, 64, device=dev)   # zero-padded to the buffer width for the GEMMs
    w0[:, :d_pe], ws[:, :d_pe] = r(h, d_pe) / h ** 0.5, r(h, d_pe) / h ** 0.5
    g1, g2 = r(n, 64), r(n, 64)
    coef = -torch.tensor([4.0 ** f for f in range(n_freqs) for _ in range(6)], device=dev)
    buf = torch.empty(n, 64, device=dev)

    def kernel():
        return hip.geo_point_grad(p, n_freqs, 1.0, dz0, w0, dzs=dzs, ws=ws, g_pe=g1, g_pe2=g2, d_grad=d_grad)

    def composed():
        hip.gemm(dz0, w0, out=buf)
        hip.gemm(dzs, ws, out=buf, epi=hip.EPI_ACCUM)
        d_p = hip.pe_encode_bwd(p, buf, n_freqs, 1.0)
        pe = hip.pe_encode(p, n_freqs, 64, 1.0)
        hs = ((g1[:, 3:d_pe] + g2[:, 3:d_pe]) * pe[:, 3:d_pe] * coef).view(n, 2 * n_freqs, 3).sum(1)
        return d_p + d_grad * hs
    a, b = kernel(), composed()
    inner = 20 if n <= 20000 else 4
    res = {'rows': n, 'h0': h, 'hs': h, 'n_freqs': n_freqs, 'launches_composed': '2 gemm + pe_encode_bwd + pe_encode + 5 torch ops',
           'max_abs_difference': float((a - b).abs().max()), 'max_abs_value': float(b.abs().max()),
           'kernel': _timed(kernel, repeats, warmup, inner), 'composed': _timed(composed, repeats, warmup, inner)}
    res['kernel_over_composed'] = res['kernel']['median_ms'] / res['composed']['median_ms']
    # bytes the kernel must read and write: both dz blocks, the two g_pe pieces (d_pe columns), p, d_grad, d_p
    res['kernel_bytes'] = n * 4 * (2 * h + 2 * d_pe + 9)
    res['kernel_gb_per_s'] = res['kernel_bytes'] / res['kernel']['median_ms'] * 1e-6
    res['kernel_tflops'] = 2.0 * n * 2 * h * 48 / res['kernel']['median_ms'] * 1e-9   # the MFMAs issued (d_pe padded to 48)
    return res


def bench_step(net, dev, repeats, warmup, max_faces=10000):
    """One refinement step on the shipped extraction's mesh; events around the field's forward and (by autograd hooks) backward."""
    from psnerf_amd.stage1 import extracting
    mesh, _ = extracting.Extractor3D(net, device=dev, resolution0=64, upsampling_steps=3).generate_mesh()
    v = torch.nn.Parameter(torch.as_tensor(mesh.vertices, dtype=torch.float32).to(dev))
    faces = torch.as_tensor(mesh.faces).to(dev)
    opt = torch.optim.RMSprop([v], lr=1e-5)
    rng = np.random.RandomState(0)
    ev = {}
    mark = lambda k: ev.setdefault(k, []).append(_now())
    real = net._geo_call

    def geo_call(q, *a, **k):
        mark('f0')
        out = real(q, *a, **k)
        mark('f1')
        for t in (out[0], out[2]):
            t.register_hook(lambda g: (mark('b0'), g)[1])
        q.register_hook(lambda g: (mark('b1'), g)[1])
        return out
    net._geo_call = geo_call
    runs = []
    try:
        for it in range(warmup + repeats):
            ev.clear()
            f_it = faces[torch.as_tensor(rng.permutation(faces.shape[0])[:max_faces]).to(dev)]
            eps = torch.as_tensor(rng.dirichlet((0.5, 0.5, 0.5), size=f_it.shape[0]), dtype=torch.float32).to(dev)
            torch.cuda.synchronize()
            mark('s0')
            opt.zero_grad()
            loss = extracting.refine_loss(net, v, f_it, eps, 0.5)[0]
            loss.backward()
            opt.step()
            mark('s1')
            torch.cuda.synchronize()
            if it >= warmup:
                total, fwd = ev['s0'][0].elapsed_time(ev['s1'][0]), ev['f0'][0].elapsed_time(ev['f1'][0])
                bwd = ev['b0'][-1].elapsed_time(ev['b1'][0])   # from the LAST of the two output gradients to d / dp
                runs.append((total, fwd, bwd, total - fwd - bwd))
    finally:
        del net._geo_call
    names = ('step', 'field_forward', 'field_backward', 'rest')
    res = {n: _stat([r[i] for r in runs]) for i, n in enumerate(names)}
    res.update(vertices=int(v.shape[0]), faces=int(faces.shape[0]), faces_per_step=int(min(max_faces, faces.shape[0])))
    return res


def _now():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def bench_engine(net, dev, repeats, warmup, Q=262144):
    from psnerf_amd import ops
    g = torch.Generator().manual_seed(1)
    pts = ((torch.rand(Q, 3, generator=g) - 0.5) * 1.6).to(dev)
    c = [torch.randn(Q, k, generator=g).to(dev) for k in (1, 256, 3)]
    res = {'points': Q}
    for key, need in (('p_without_gradient', False), ('p_with_gradient', True)):
        def run():
            params = net._geo_params()
            p = pts.clone().requires_grad_(need)
            logit, feat, grad = ops.GeoFieldFused.apply(p, net.octaves_pe, 1.0 / net.rescale, tuple(net.skips), True, net._geo_chains(params),
                                                        None, *params)
            ((logit * c[0]).sum() + (feat * c[1]).sum() + (grad * c[2]).sum()).backward()
            net.zero_grad(set_to_none=True)
        res[key] = _timed(run, repeats, warmup)
    res['cost_of_d_p_ms'] = res['p_with_gradient']['median_ms'] - res['p_without_gradient']['median_ms']
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_refine.json'))
    args = ap.parse_args(argv)
    from psnerf_amd.stage1 import NeuralNetwork
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = NeuralNetwork(stage1_cfg('bear')).to(dev).eval()
    out = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'warmup': args.warmup,
           'a_point_grad_kernel': [bench_kernel(n, dev, args.repeats, args.warmup) for n in (10000, 262144)],
           'b_refinement_step': bench_step(net, dev, args.repeats, args.warmup),
           'c_geo_field_fused_fwd_bwd': bench_engine(net, dev, args.repeats, args.warmup)}
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, sort_keys=True))
    return args.out


if __name__ == '__main__':
    main()
