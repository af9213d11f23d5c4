"""Stage-1 product path (HIP) against golden vectors captured from the reference and the CPU oracle."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import (ATOL_DEPTH, ATOL_LOGIT, ATOL_NORMAL, ATOL_UNIT, COMPUTE_LOSS_CASES, GOLDEN, assert_close, compute_loss_case, grad_digest,
                           stage1_state_dict, state_dict_digest, stage1_cfg)

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize('tag,over', [('h64', {'model.hidden_dim': 64, 'model.feat_size': 64}), ('h256', {})])
def test_network_golden(cuda, tag, over):
    from psnerf_amd.stage1 import NeuralNetwork
    g = np.load(os.path.join(GOLDEN, 'stage1_net_%s.npz' % tag))
    cfg = stage1_cfg('bunny', **over)
    sd = stage1_state_dict(cfg, seed=11)
    assert state_dict_digest(sd) == str(g['sd_digest'])
    net = NeuralNetwork(cfg)
    net.load_state_dict(sd)
    net.to(cuda)
    p, ray_d = T(g['p'], cuda), T(g['ray_d'], cuda)
    occ = net.infer_occ(p.clone())
    grad = net.gradient(p.clone())[:, 0]
    rgb, alpha = net(p.clone(), ray_d, return_addocc=True)
    # elementwise |a - b| <= 1e-4 |b| + atol (tests/helpers.py: the floors per output class)
    assert_close(occ.detach().cpu(), g['occ'], 1e-4, 'occ', atol=ATOL_LOGIT)
    assert_close(grad.detach().cpu(), g['grad'], 1e-4, 'grad', atol=ATOL_LOGIT)
    assert_close(rgb.detach().cpu(), g['rgb'], 1e-4, 'rgb', atol=ATOL_UNIT)
    assert_close(alpha.detach().cpu(), g['alpha'], 1e-4, 'alpha', atol=ATOL_UNIT)
    with torch.no_grad():
        assert_close(net(p, only_occupancy=True).cpu(), g['occ_only'], 1e-4, 'occ_only (fused or GEMM path)', atol=ATOL_UNIT)
        assert_close(net(p, return_logits=True).cpu(), g['logits'], 1e-4, 'logits', atol=ATOL_LOGIT)
    loss = (rgb * T(g['c_rgb'], cuda)).sum() + (alpha * T(g['c_alpha'], cuda)).sum() \
        + (occ * T(g['c_occ'], cuda)).sum() * 0.01 + (grad * T(g['c_grad'], cuda)).sum() * 0.1
    loss.backward()
    assert_close(float(loss.detach()), float(g['loss']), 1e-4, 'loss', atol=0.0)
    names, norms, projs = grad_digest({k: v.grad for k, v in net.named_parameters()})
    assert names == list(g['grad_names'])
    if tag == 'h64':
        for k, v in net.named_parameters():
            assert_close(v.grad.cpu(), g['g_' + k], 1e-3, 'grad ' + k)
    assert_close(norms, g['grad_norms'], 1e-3, 'grad norms')
    assert_close(projs, g['grad_projs'], 2e-3, 'grad projs')


def test_geo_chains_vs_gemm_path(cuda):
    """The fused register-resident chains (ops.GeoFieldFused) and the GEMM sequence (ops.GeoField) are two
    implementations of the same double-backward: every parameter gradient must agree."""
    from psnerf_amd.stage1 import NeuralNetwork
    g = np.load(os.path.join(GOLDEN, 'stage1_net_h256.npz'))
    cfg = stage1_cfg('bunny')
    sd = stage1_state_dict(cfg, seed=11)
    res = {}
    for fusedp in (True, False):
        net = NeuralNetwork(cfg)
        net.load_state_dict(sd)
        net.to(cuda)
        net.USE_FUSED_CHAINS = fusedp
        p, ray_d = T(g['p'], cuda), T(g['ray_d'], cuda)
        rgb, alpha = net(p.clone(), ray_d, return_addocc=True)
        grad = net.gradient(p.clone())[:, 0]
        loss = (rgb * T(g['c_rgb'], cuda)).sum() + (alpha * T(g['c_alpha'], cuda)).sum() \
            + (grad * T(g['c_grad'], cuda)).sum() * 0.1
        loss.backward()
        res[fusedp] = (rgb.detach().cpu(), grad.detach().cpu(), {k: v.grad.cpu() for k, v in net.named_parameters()})
    assert_close(res[True][0], res[False][0], 1e-5, 'rgb')
    assert_close(res[True][1], res[False][1], 1e-4, 'grad')
    for k in res[True][2]:
        assert_close(res[True][2][k], res[False][2][k], 1e-3, 'param grad ' + k)


def test_network_state_dict_and_init(cuda):
    """Same seed -> same initial weights as the reference (digest captured by tools/gen_golden.py)."""
    from psnerf_amd.stage1 import NeuralNetwork
    g = np.load(os.path.join(GOLDEN, 'stage1_net_h256.npz'))
    torch.manual_seed(7)
    net = NeuralNetwork(stage1_cfg('bunny'))
    assert state_dict_digest(net.state_dict()) == str(g['init_digest'])
    assert sum(p.numel() for p in net.parameters()) == 802490


def _renderer(cuda):
    from psnerf_amd.stage1 import NeuralNetwork, Renderer
    cfg = stage1_cfg('bunny')
    net = NeuralNetwork(cfg)
    net.load_state_dict(stage1_state_dict(cfg, seed=11))
    return cfg, net, Renderer(net, cfg, device=cuda)


def test_march_and_light_visibility_golden(cuda):
    from psnerf_amd.stage1.rendering import camera_origin, pixel_rays
    g = np.load(os.path.join(GOLDEN, 'stage1_march.npz'))
    cfg, net, ren = _renderer(cuda)
    pix, K, c2w = T(g['pix'], cuda), T(g['K'], cuda), T(g['c2w'], cuda)
    N = pix.shape[1]
    cam = camera_origin(N, c2w)
    rays = pixel_rays(pix, K, c2w)
    rays = rays / rays.norm(2, 2).unsqueeze(-1)
    d = ren.ray_marching(cam, rays, n_steps=[256, 257], n_secant_steps=8, rad=2.0, depth_range=[2, 6]).cpu()
    ref = torch.from_numpy(g['d_i'])
    fin = torch.isfinite(ref)
    assert torch.equal(fin, torch.isfinite(d)), 'hit / miss classification differs'
    assert torch.equal(ref == 0, d == 0)
    assert_close(d[fin], ref[fin], 1e-4, 'd_i', atol=ATOL_DEPTH)
    lv = ren.light_visibility(surf=T(g['surf'], cuda), light_dir=T(g['ldir'], cuda)).cpu()
    assert_close(lv, g['light_vis'], 1e-4, 'light visibility', atol=ATOL_UNIT)


@pytest.mark.parametrize('tag', ['it0', 'it6000', 'cfg1'])
def test_unisurf_golden(cuda, tag):
    """G6 against the reference's own Renderer.unisurf + Loss + backward ('cfg1': 512 rays x 64 samples, 256 march steps = the
    scale of BASELINE configs[0])."""
    from psnerf_amd.stage1 import Loss
    g = np.load(os.path.join(GOLDEN, 'stage1_unisurf_%s.npz' % tag))
    it = int(g['it'])
    cfg, net, ren = _renderer(cuda)
    noise = {'miss': T(g['nz_miss'], cuda), 'hit': T(g['nz_hit'], cuda), 'nbr': T(g['nz_nbr'], cuda)}
    out = ren(T(g['pix'], cuda), T(g['K'], cuda), T(g['c2w'], cuda), torch.eye(4, device=cuda)[None], 'unisurf',
              add_noise=True, eval_=False, it=it, noise=noise)
    assert np.array_equal(out['mask_pred'].cpu().numpy(), g['mask_pred'])
    for k in ('rgb', 'normal_pred', 'acc_map'):
        # cfg1 (512 rays): a near-zero COMPONENT of a unit normal is bounded on the vector's scale -- 1e-5 absolute = 1e-5 of its length
        # (the oracle itself sits 4.8e-6 from the reference on the worst of these 1536 components, tools/gen_golden.py)
        assert_close(out[k].detach().cpu(), g[k], 1e-4, k, atol=1e-5 if (tag == 'cfg1' and k == 'normal_pred') else ATOL_UNIT)
    # diff_norm is a difference of nearly equal unit normals: compare on the normals' scale (1.0)
    assert float(np.abs(out['diff_norm'].detach().cpu().numpy() - g['diff_norm']).max()) < 1e-4
    terms = Loss(1.0, 0.005, 0.05, 1.0, device=cuda)(out, T(g['rgb_gt'], cuda), T(g['normal_gt'], cuda),
                                                     T(g['norm_mask'], cuda))
    for k, v in zip(g['loss_names'], g['loss_vals']):
        assert_close(float(terms[str(k)].detach()), v, 1e-3 if str(k) == 'grad_loss' else 1e-4, str(k), atol=0.0)
    terms['loss'].backward()
    names, norms, projs = grad_digest({k: v.grad for k, v in net.named_parameters()})
    assert names == list(g['grad_names'])
    assert_close(norms, g['grad_norms'], 1e-3, 'grad norms')
    assert_close(projs, g['grad_projs'], 2e-3, 'grad projs')


def test_unisurf_eval_and_shape_extract_vs_oracle(cuda):
    """eval_ path (no noise, no graph) and shape_extract with shadow-ray visibility against the oracle."""
    from oracle import stage1 as o1
    from psnerf_amd.synthetic import stage1_camera
    cfg, net, ren = _renderer(cuda)
    onet = o1.NeuralNetwork(cfg)
    onet.load_state_dict(stage1_state_dict(cfg, seed=11))
    oren = o1.Renderer(onet, cfg)
    h, w = 48, 64
    K, c2w, S = stage1_camera(cfg, h=h, w=w)
    gen = torch.Generator().manual_seed(3)
    pix = torch.stack([torch.randint(0, w, (150,), generator=gen).float(),
                       torch.randint(0, h, (150,), generator=gen).float()], -1)[None]
    with torch.no_grad():
        o = oren(pix, K, c2w, S, 'unisurf', add_noise=False, eval_=True, it=0)
        p = ren(pix.to(cuda), K.to(cuda), c2w.to(cuda), S.to(cuda), 'unisurf', add_noise=False, eval_=True, it=0)
    assert torch.equal(o['mask_pred'], p['mask_pred'].cpu())
    for k in ('rgb', 'normal_pred', 'acc_map'):
        assert_close(p[k].cpu(), o[k], 1e-4, k, atol=ATOL_UNIT)
    ldir = torch.nn.functional.normalize(torch.randn(5, 3, generator=gen), dim=-1)
    o = oren(pix, K, c2w, S, 'shape_extract', visibility=True, light_dir=ldir)
    p = ren(pix.to(cuda), K.to(cuda), c2w.to(cuda), S.to(cuda), 'shape_extract', visibility=True, light_dir=ldir.to(cuda))
    assert torch.equal(o['mask'], p['mask'].cpu())
    for k in ('normal', 'points', 'visibility'):
        assert_close(p[k].cpu(), o[k], 1e-4, k, atol=ATOL_DEPTH if k == 'points' else ATOL_UNIT)


def test_train_step_vs_oracle(cuda):
    """Full stage-1 train step (march + render + loss + backward + Adam) vs the oracle, 2 iterations."""
    from oracle import stage1 as o1
    from psnerf_amd.stage1 import NeuralNetwork, Renderer, Trainer
    from psnerf_amd.synthetic import stage1_batch
    cfg = stage1_cfg('bunny', **{'training.n_training_points': 128})
    sd = stage1_state_dict(cfg, seed=21)
    onet = o1.NeuralNetwork(cfg)
    onet.load_state_dict(sd)
    otr = o1.Trainer(o1.Renderer(onet, cfg), torch.optim.Adam(onet.parameters(), lr=1e-4), cfg)
    net = NeuralNetwork(cfg)
    net.load_state_dict(sd)
    ren = Renderer(net, cfg, device=cuda)
    tr = Trainer(ren, torch.optim.Adam(net.parameters(), lr=1e-4), cfg, device=cuda)
    batch = stage1_batch(cfg, h=48, w=64, seed=4)
    for it in (1000, 1001):
        gen = torch.Generator().manual_seed(it)
        pix = torch.stack([torch.randint(0, 64, (128,), generator=gen).float(),
                           torch.randint(0, 48, (128,), generator=gen).float()], -1)[None]
        # discover the hit count with a dry march so both sides get identical injected noise
        with torch.no_grad():
            dry = o1.Renderer(onet, cfg)(pix, batch['img.camera_mat'], batch['img.world_mat'], batch['img.scale_mat'],
                                         'unisurf', add_noise=False, eval_=True, it=it)
        n_hit = int(dry['mask_pred'].sum())
        S_ = 64
        noise = {'miss': torch.rand(1, 128 - n_hit, S_, generator=gen), 'hit': torch.rand(1, n_hit, S_, generator=gen),
                 'nbr': torch.rand(n_hit, 3, generator=gen)}
        ot = otr.train_step(batch, it=it, pix=pix, noise=noise)
        pt = tr.train_step(batch, it=it, pix=pix, noise={k: v.to(cuda) for k, v in noise.items()})
        for k in ot:
            assert_close(float(pt[k].detach()), float(ot[k].detach()), 1e-3 if k == 'grad_loss' else 2e-4, '%s it%d' % (k, it), atol=0.0)
    osd = onet.state_dict()
    # (with lr = 1e-4 two Adam steps move no element by more than about 2e-4, so the maximum bound below is implied by the
    #  learning rate whatever the gradient is and only the mean bound carries information: the correctness of the gradients
    #  themselves is gated, parameter by parameter against float64, in tests/test_step1_grad_gpu.py)
    for k, v in net.state_dict().items():
        d = (v.cpu() - osd[k]).abs()
        assert float(d.max()) <= 2 * 2 * 1e-4 + 1e-6, 'param %s max diff %.3e' % (k, float(d.max()))
        assert float(d.mean()) <= 1e-5, 'param %s mean diff %.3e' % (k, float(d.mean()))


def test_sync_free_training_forward_matches_reference_shaped_path(cuda, monkeypatch):
    """Renderer._unisurf_sync_free (both ray groups in one flagged sampling launch, normals of every ray masked, loss
    denominators on the device) against the reference-shaped path (index lists, compact diff_norm, host counts): same
    outputs, same loss terms, same parameter gradients -- with the random offsets pinned to a constant in both."""
    from psnerf_amd.stage1 import Loss, NeuralNetwork, Renderer
    from psnerf_amd.synthetic import stage1_camera
    monkeypatch.setattr(torch, 'rand_like', lambda t, **k: torch.full_like(t, 0.75))
    cfg = stage1_cfg('bunny')
    sd = stage1_state_dict(cfg, seed=11)
    h, w = 48, 64
    K, c2w, S = stage1_camera(cfg, h=h, w=w)
    gen = torch.Generator().manual_seed(5)
    n = 200
    pix = torch.stack([torch.randint(0, w, (n,), generator=gen).float(), torch.randint(0, h, (n,), generator=gen).float()], -1)[None].to(cuda)
    rgb_gt = torch.rand(1, n, 3, generator=gen).to(cuda)
    ngt = torch.nn.functional.normalize(torch.randn(1, n, 3, generator=gen), dim=-1).to(cuda)
    nmask = (torch.rand(1, n, generator=gen) > 0.3).to(cuda)
    res = []
    for it in (100, 6000):
        pair = []
        for sync_free in (False, True):
            net = NeuralNetwork(cfg)
            net.load_state_dict(sd)
            ren = Renderer(net, cfg, device=cuda)
            ren.sync_free = sync_free
            out = ren(pix, K.to(cuda), c2w.to(cuda), S.to(cuda), 'unisurf', add_noise=False, eval_=False, it=it)
            assert (out.get('diff_norm_full') is not None) == sync_free
            terms = Loss(1.0, 0.005, 0.05, 1.0, device=cuda)(out, rgb_gt, ngt, nmask)
            terms['loss'].backward()
            pair.append((out, terms, {k: v.grad.clone() for k, v in net.named_parameters()}))
        (o0, t0, g0), (o1, t1, g1) = pair
        assert torch.equal(o0['mask_pred'], o1['mask_pred']) and int(o0['mask_pred'].sum()) > 0
        for k in ('rgb', 'acc_map', 'normal_pred'):
            assert_close(o1[k].detach().cpu(), o0[k].detach().cpu(), 1e-6, '%s it%d' % (k, it), atol=ATOL_UNIT)
        hit = o0['mask_pred']
        assert_close(o1['diff_norm_full'][hit].detach().cpu(), o0['diff_norm'].detach().cpu(), 1e-5, 'diff_norm it%d' % it, atol=1e-7)
        for k in t0:
            assert_close(float(t1[k].detach()), float(t0[k].detach()), 1e-5, '%s it%d' % (k, it), atol=0.0)
        for k in g0:
            assert_close(g1[k].cpu(), g0[k].cpu(), 1e-4, 'grad %s it%d' % (k, it))


@pytest.mark.parametrize('case', ['all_miss', 'all_hit'])
def test_sync_free_forward_on_batches_without_hits_or_without_misses_vs_oracle(cuda, case):
    """Edge cases of the training forward (rendering.py:84-108: the hit / miss split): a batch in which EVERY ray misses the object
    (the hit group of the reference is empty: no surface points, no normals, diff_norm of zero rows, grad_loss = 0) and one in which
    every ray hits (the miss group is empty).  The sync-free forward has no groups -- one flagged launch over all rays, masked
    normals, device-side counts -- and must still give the oracle's outputs, loss terms and parameter gradients."""
    from oracle import stage1 as o1
    from psnerf_amd.stage1 import Loss, NeuralNetwork, Renderer
    from psnerf_amd.stage1.rendering import sync_free_noise_for_reference
    from psnerf_amd.synthetic import stage1_camera
    cfg = stage1_cfg('bunny')
    sd = stage1_state_dict(cfg, seed=11)
    h, w = 48, 64
    K, c2w, S = stage1_camera(cfg, h=h, w=w)
    onet = o1.NeuralNetwork(cfg)
    onet.load_state_dict(sd)
    oren = o1.Renderer(onet, cfg)
    # classify every pixel once with the oracle, then draw the batch from one class only
    ys, xs = torch.meshgrid(torch.arange(0, h, 2).float(), torch.arange(0, w, 2).float(), indexing='ij')   # (every second pixel: 768 rays on the CPU)
    grid = torch.stack([xs.reshape(-1), ys.reshape(-1)], -1)[None]
    with torch.no_grad():
        mask_all = oren(grid, K, c2w, S, 'unisurf', add_noise=False, eval_=True, it=100)['mask_pred']
    pool = grid[0][mask_all if case == 'all_hit' else ~mask_all]
    assert pool.shape[0] >= 96, (case, pool.shape)
    gen = torch.Generator().manual_seed(7)
    n = 96
    pix = pool[torch.randperm(pool.shape[0], generator=gen)[:n]][None]
    rgb_gt = torch.rand(1, n, 3, generator=gen)
    ngt = torch.nn.functional.normalize(torch.randn(1, n, 3, generator=gen), dim=-1)
    nmask = torch.rand(1, n, generator=gen) > 0.3
    it = 100
    noise = {'full': torch.rand(n, 64, generator=gen), 'nbr_full': torch.rand(n, 3, generator=gen)}
    net = NeuralNetwork(cfg)
    net.load_state_dict(sd)
    ren = Renderer(net, cfg, device=cuda)
    ren.sync_free = True
    out = ren(pix.to(cuda), K.to(cuda), c2w.to(cuda), S.to(cuda), 'unisurf', add_noise=True, eval_=False, it=it,
              noise={k: v.to(cuda) for k, v in noise.items()})
    hit = out['mask_pred'].cpu()
    assert int(hit.sum()) == (n if case == 'all_hit' else 0)
    o = oren(pix, K, c2w, S, 'unisurf', add_noise=True, eval_=False, it=it, noise=sync_free_noise_for_reference(noise, hit))
    assert torch.equal(o['mask_pred'], hit)
    for k in ('rgb', 'normal_pred', 'acc_map'):
        assert_close(out[k].detach().cpu(), o[k].detach(), 1e-4, k, atol=ATOL_NORMAL if k == 'normal_pred' else ATOL_UNIT)
    terms = Loss(1.0, 0.005, 0.05, 1.0, device=cuda)(out, rgb_gt.to(cuda), ngt.to(cuda), nmask.to(cuda))
    oterms = o1.Loss(1.0, 0.005, 0.05, 1.0)(o, rgb_gt, ngt, nmask)
    assert sorted(terms) == sorted(oterms)
    for k in oterms:
        assert_close(float(terms[k].detach()), float(oterms[k].detach()), 1e-3 if k == 'grad_loss' else 1e-4, k, atol=1e-12)
    if case == 'all_miss':
        assert float(terms['grad_loss'].detach()) == 0.0 and float(oterms['grad_loss']) == 0.0
    terms['loss'].backward()
    oterms['loss'].backward()
    og = {k: v.grad for k, v in onet.named_parameters()}
    for k, v in net.named_parameters():
        if og[k] is None:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
        else:
            assert_close(v.grad.cpu(), og[k], 1e-3, 'grad ' + k)


@pytest.mark.parametrize('it', [100, 6000])
def test_sync_free_forward_with_jitter_vs_oracle(cuda, it):
    """The forward the bench and the Trainer actually run -- Renderer._unisurf_sync_free: one flagged sampling launch, one
    [N, S] jitter table, normals of every ray -- against the ORACLE with the stratified jitter ON: the per-ray tables are
    split by the hit mask into the group-sized tables of the reference's draw order (sync_free_noise_for_reference), so
    both sides use the same draw for the same (ray, sample).  Outputs, loss terms and every parameter gradient."""
    from oracle import stage1 as o1
    from psnerf_amd.stage1 import Loss, NeuralNetwork, Renderer
    from psnerf_amd.stage1.rendering import sync_free_noise_for_reference
    from psnerf_amd.synthetic import stage1_camera
    cfg = stage1_cfg('bunny')
    sd = stage1_state_dict(cfg, seed=11)
    h, w = 48, 64
    K, c2w, S = stage1_camera(cfg, h=h, w=w)
    gen = torch.Generator().manual_seed(50 + it)
    n = 200
    pix = torch.stack([torch.randint(0, w, (n,), generator=gen).float(), torch.randint(0, h, (n,), generator=gen).float()], -1)[None]
    rgb_gt = torch.rand(1, n, 3, generator=gen)
    ngt = torch.nn.functional.normalize(torch.randn(1, n, 3, generator=gen), dim=-1)
    nmask = torch.rand(1, n, generator=gen) > 0.3
    full_steps = 96 if it > 5000 else 64
    noise = {'full': torch.rand(n, full_steps, generator=gen), 'nbr_full': torch.rand(n, 3, generator=gen)}
    net = NeuralNetwork(cfg)
    net.load_state_dict(sd)
    ren = Renderer(net, cfg, device=cuda)
    ren.sync_free = True
    out = ren(pix.to(cuda), K.to(cuda), c2w.to(cuda), S.to(cuda), 'unisurf', add_noise=True, eval_=False, it=it,
              noise={k: v.to(cuda) for k, v in noise.items()})
    assert out.get('diff_norm_full') is not None and out['diff_norm'] is None, 'not the sync-free forward'
    hit = out['mask_pred'].cpu()
    assert 20 < int(hit.sum()) < n - 20
    onet = o1.NeuralNetwork(cfg)
    onet.load_state_dict(sd)
    o = o1.Renderer(onet, cfg)(pix, K, c2w, S, 'unisurf', add_noise=True, eval_=False, it=it,
                               noise=sync_free_noise_for_reference(noise, hit))
    assert torch.equal(o['mask_pred'], hit)
    for k in ('rgb', 'normal_pred', 'acc_map'):
        assert_close(out[k].detach().cpu(), o[k].detach(), 1e-4, k, atol=ATOL_NORMAL if k == 'normal_pred' else ATOL_UNIT)
    # diff_norm is a difference of nearly equal unit normals: compare on the normals' scale (1.0)
    assert float((out['diff_norm_full'].detach().cpu()[hit] - o['diff_norm'].detach()).abs().max()) < 1e-4
    terms = Loss(1.0, 0.005, 0.05, 1.0, device=cuda)(out, rgb_gt.to(cuda), ngt.to(cuda), nmask.to(cuda))
    oterms = o1.Loss(1.0, 0.005, 0.05, 1.0)(o, rgb_gt, ngt, nmask)
    assert sorted(terms) == sorted(oterms)
    for k in oterms:
        assert_close(float(terms[k].detach()), float(oterms[k].detach()), 1e-3 if k == 'grad_loss' else 1e-4, k, atol=0.0)
    terms['loss'].backward()
    oterms['loss'].backward()
    names, norms, projs = grad_digest({k: v.grad for k, v in net.named_parameters()})
    onames, onorms, oprojs = grad_digest({k: v.grad for k, v in onet.named_parameters()})
    assert names == onames
    assert_close(norms, onorms, 1e-3, 'grad norms')
    assert_close(projs, oprojs, 2e-3, 'grad projs')
    # the same tables through the reference-shaped path of the product (index lists, compact diff_norm): same rays, same draws
    net2 = NeuralNetwork(cfg)
    net2.load_state_dict(sd)
    ren2 = Renderer(net2, cfg, device=cuda)
    with torch.no_grad():
        out2 = ren2(pix.to(cuda), K.to(cuda), c2w.to(cuda), S.to(cuda), 'unisurf', add_noise=True, eval_=False, it=it,
                    noise={k: v.to(cuda) for k, v in noise.items()})
    assert out2['diff_norm'] is not None
    for k in ('rgb', 'acc_map', 'normal_pred'):
        assert_close(out2[k].cpu(), out[k].detach().cpu(), 1e-6, 'reference-shaped vs sync-free ' + k, atol=ATOL_UNIT)


def test_sync_free_train_steps_vs_oracle_with_jitter(cuda):
    """Trainer.train_step on its default (sync-free) path, jitter ON, two Adam steps across nothing but the per-ray tables:
    loss terms and parameters after the steps against the oracle's Trainer."""
    from oracle import stage1 as o1
    from psnerf_amd.stage1 import NeuralNetwork, Renderer, Trainer
    from psnerf_amd.stage1.rendering import sync_free_noise_for_reference
    from psnerf_amd.synthetic import stage1_batch
    cfg = stage1_cfg('bunny', **{'training.n_training_points': 128})
    sd = stage1_state_dict(cfg, seed=21)
    onet = o1.NeuralNetwork(cfg)
    onet.load_state_dict(sd)
    otr = o1.Trainer(o1.Renderer(onet, cfg), torch.optim.Adam(onet.parameters(), lr=1e-4), cfg)
    net = NeuralNetwork(cfg)
    net.load_state_dict(sd)
    ren = Renderer(net, cfg, device=cuda)
    tr = Trainer(ren, torch.optim.Adam(net.parameters(), lr=1e-4), cfg, device=cuda)
    calls = []
    inner = ren._unisurf_sync_free
    ren._unisurf_sync_free = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    batch = stage1_batch(cfg, h=48, w=64, seed=4)
    for it in (1000, 1001):
        gen = torch.Generator().manual_seed(it)
        pix = torch.stack([torch.randint(0, 64, (128,), generator=gen).float(),
                           torch.randint(0, 48, (128,), generator=gen).float()], -1)[None]
        with torch.no_grad():  # the hit mask of the CURRENT weights splits the per-ray tables for the oracle
            dry = o1.Renderer(onet, cfg)(pix, batch['img.camera_mat'], batch['img.world_mat'], batch['img.scale_mat'],
                                         'unisurf', add_noise=False, eval_=True, it=it)
        noise = {'full': torch.rand(128, 64, generator=gen), 'nbr_full': torch.rand(128, 3, generator=gen)}
        ot = otr.train_step(batch, it=it, pix=pix, noise=sync_free_noise_for_reference(noise, dry['mask_pred']))
        pt = tr.train_step(batch, it=it, pix=pix, noise={k: v.to(cuda) for k, v in noise.items()})
        assert sorted(ot) == sorted(pt)
        for k in ot:
            assert_close(float(pt[k].detach()), float(ot[k].detach()), 1e-3 if k == 'grad_loss' else 2e-4, '%s it%d' % (k, it), atol=0.0)
    assert len(calls) == 2, 'the trainer did not take the sync-free forward'
    osd = onet.state_dict()
    # (with lr = 1e-4 two Adam steps move no element by more than about 2e-4, so the maximum bound below is implied by the
    #  learning rate whatever the gradient is and only the mean bound carries information: the correctness of the gradients
    #  themselves is gated, parameter by parameter against float64, in tests/test_step1_grad_gpu.py)
    for k, v in net.state_dict().items():
        d = (v.cpu() - osd[k]).abs()
        assert float(d.max()) <= 2 * 2 * 1e-4 + 1e-6, 'param %s max diff %.3e' % (k, float(d.max()))
        assert float(d.mean()) <= 1e-5, 'param %s mean diff %.3e' % (k, float(d.mean()))


def test_shape_extract_golden(cuda):
    """Renderer.shape_extract on an int64 x-major pixel chunk with shadow-ray visibility (stage1/shape_extract.py:112-139)
    against the reference's own outputs (tests/golden/stage1_shape_extract.npz)."""
    g = np.load(os.path.join(GOLDEN, 'stage1_shape_extract.npz'))
    cfg, net, ren = _renderer(cuda)
    assert state_dict_digest(stage1_state_dict(cfg, seed=11)) == str(g['sd_digest'])
    pix = T(g['pix'], cuda)
    assert pix.dtype == torch.int64
    out = ren(pix, T(g['K'], cuda), T(g['c2w'], cuda), torch.eye(4, device=cuda)[None], 'shape_extract', visibility=True,
              light_dir=T(g['ldir'], cuda))
    assert np.array_equal(out['mask'].cpu().numpy(), g['mask'])
    assert_close(out['normal'].cpu(), g['normal'], 1e-4, 'normal', atol=ATOL_NORMAL)
    assert_close(out['points'].cpu(), g['points'], 1e-4, 'points', atol=ATOL_DEPTH)
    assert_close(out['visibility'].cpu(), g['visibility'], 1e-4, 'visibility', atol=ATOL_UNIT)


def test_phong_renderer_golden(cuda):
    """Renderer.forward(..., 'phong_renderer') (rendering.py:228-293: the third rendering_technique, the shaded preview of
    training.py:62-118) against the reference's own method (tests/golden/stage1_phong.npz): background pixels exactly 1, surface
    pixels 0.3 + 0.7 max(n . l, 0) with the normal of a root-found point (its floor: ATOL_NORMAL x 0.7)."""
    g = np.load(os.path.join(GOLDEN, 'stage1_phong.npz'))
    cfg, net, ren = _renderer(cuda)
    assert state_dict_digest(stage1_state_dict(cfg, seed=11)) == str(g['sd_digest'])
    out = ren(T(g['pix'], cuda).float(), T(g['K'], cuda), T(g['c2w'], cuda), torch.eye(4, device=cuda)[None], 'phong_renderer')
    assert sorted(out) == ['rgb'] and out['rgb'].shape == g['rgb'].shape
    bg = (g['rgb'] == 1).all(-1)
    assert np.array_equal((out['rgb'].cpu().numpy() == 1).all(-1), bg) and 10 < int((~bg).sum()) < 200
    assert_close(out['rgb'].cpu(), g['rgb'], 1e-4, 'rgb', atol=ATOL_NORMAL)


def test_render_visdata_golden(cuda, tmp_path):
    """Trainer.render_visdata (stage1/model/training.py:62-118: the periodic image grid -- input | rgb | normal | normal map | angular
    error | mask | acc | phong preview, two items) against the image the reference's OWN method wrote (tests/golden/
    stage1_visdata.npz; uint8): rendered in ONE chunk here against the reference's 1024-pixel chunks.  A quantised 8-bit panel can
    differ by one level where a value sits on a rounding edge, and a silhouette pixel may flip: >= 99 % of the values within one
    level, mean absolute difference < 0.5 levels; the file is written and holds the returned array."""
    from PIL import Image
    from psnerf_amd.stage1 import NeuralNetwork, Renderer, Trainer
    from psnerf_amd.synthetic import stage1_batch
    g = np.load(os.path.join(GOLDEN, 'stage1_visdata.npz'))
    cfg, net, ren = _renderer(cuda)
    assert state_dict_digest(stage1_state_dict(cfg, seed=11)) == str(g['sd_digest'])
    hv, wv = (int(v) for v in g['hw'])
    items = [stage1_batch(cfg, h=hv, w=wv, seed=int(s_)) for s_ in g['seeds']]
    tr = Trainer(ren, None, cfg, device=cuda)
    out = tmp_path / 'vis.png'
    grid = tr.render_visdata(items, int(g['it']), str(out))
    assert grid.dtype == np.uint8 and grid.shape == g['grid'].shape == (2 * hv, 8 * wv, 3)
    assert np.array_equal(np.array(Image.open(str(out))), grid)
    d = np.abs(grid.astype(np.int32) - g['grid'].astype(np.int32))
    assert float((d <= 1).mean()) >= 0.99 and float(d.mean()) < 0.5, (float((d <= 1).mean()), float(d.mean()), int(d.max()))
    assert np.array_equal(grid[:, :wv], g['grid'][:, :wv])   # the input-image panel is data: exact
    assert net.training   # render_visdata leaves the model in training mode (training.py:117)


@pytest.mark.parametrize('tag', sorted(COMPUTE_LOSS_CASES))
def test_compute_loss_golden(cuda, tag):
    """Trainer.compute_loss against the reference's OWN Trainer (tests/golden/stage1_compute_loss.npz): training mode with
    the normal loss, eval_mode, mask loss; loss terms and parameter-gradient digests."""
    from psnerf_amd.stage1 import NeuralNetwork, Renderer, Trainer
    g = np.load(os.path.join(GOLDEN, 'stage1_compute_loss.npz'))
    cfg, data, pix, noise, it, eval_mode = compute_loss_case(g, tag)
    net = NeuralNetwork(cfg)
    net.load_state_dict(stage1_state_dict(cfg, seed=11))
    tr = Trainer(Renderer(net, cfg, device=cuda), None, cfg, device=cuda)
    assert tr.n_eval_points == tr.n_training_points == 160
    terms = tr.compute_loss(data, eval_mode=eval_mode, it=it, pix=pix, noise={k: v.to(cuda) for k, v in noise.items()})
    assert sorted(terms) == [str(k) for k in g[tag + '_loss_names']]
    for k, v in zip(g[tag + '_loss_names'], g[tag + '_loss_vals']):
        if float(v) == 0.0:  # eval_mode: no smoothness term at all (diff_norm is None, losses.py:41-44)
            assert float(terms[str(k)].detach()) == 0.0, k
            continue
        assert_close(float(terms[str(k)].detach()), v, 1e-3 if str(k) == 'grad_loss' else 1e-4, str(k), atol=0.0)
    terms['loss'].backward()
    names, norms, projs = grad_digest({k: v.grad for k, v in net.named_parameters()})
    assert names == list(g[tag + '_grad_names'])
    assert_close(norms, g[tag + '_grad_norms'], 1e-3, 'grad norms')
    assert_close(projs, g[tag + '_grad_projs'], 2e-3, 'grad projs')


@pytest.mark.parametrize('flat', [False, True])
def test_train_step_vs_reference_trainer(cuda, flat):
    """Two optimisation steps of the reference's OWN Trainer.train_step (training.py:46-60; tests/golden/stage1_train_step.npz)
    replayed by the HIP Trainer: loss terms of both steps and the parameters after them.  flat: optim.FlatAdam (one launch
    per step over flat parameter / gradient / moment buffers) instead of torch.optim.Adam."""
    from psnerf_amd.optim import FlatAdam
    from psnerf_amd.stage1 import NeuralNetwork, Renderer, Trainer
    from tests.test_oracle_golden import _stage1_train_step_golden

    def make(cfg, sd):
        net = NeuralNetwork(cfg)
        net.load_state_dict(sd)
        ren = Renderer(net, cfg, device=cuda)
        return net, Trainer(ren, (FlatAdam if flat else torch.optim.Adam)(net.parameters(), lr=1e-4), cfg, device=cuda)
    g, net, logs = _stage1_train_step_golden(make, dev=cuda)
    for j in range(2):
        for k, v in zip(g['s%d_loss_names' % j], g['s%d_loss_vals' % j]):
            assert_close(float(logs[j][str(k)].detach()), float(v), 1e-3 if (str(k) == 'grad_loss' or j > 0) else 1e-4, '%s step %d' % (k, j), atol=0.0)
    for k, v in net.state_dict().items():
        d = (v.detach().cpu().reshape(-1)[:1024] - torch.from_numpy(g['p_' + k])).abs()
        assert float(d.max()) <= 2 * 2 * 1e-4 + 1e-6, 'param %s max diff %.3e' % (k, float(d.max()))
        assert float(d.mean()) <= 1e-5, 'param %s mean diff %.3e' % (k, float(d.mean()))


def test_compute_loss_full_image_branch_fails_like_the_reference(cuda):
    """n_training_points >= h*w: the reference raises RuntimeError from grid_sample on its int64 pixel grid
    (training.py:159-165 -> common.py:195; the fixture holds its exception); so does the product, before the forward."""
    from psnerf_amd.stage1 import NeuralNetwork, Renderer, Trainer
    from psnerf_amd.synthetic import stage1_batch
    g = np.load(os.path.join(GOLDEN, 'stage1_compute_loss.npz'))
    cfg = stage1_cfg('bunny', **{'training.n_training_points': 48})
    tr = Trainer(Renderer(NeuralNetwork(cfg), cfg, device=cuda), None, cfg, device=cuda)
    with pytest.raises(RuntimeError) as e:
        tr.compute_loss(stage1_batch(cfg, h=6, w=8, seed=6), it=0)
    assert ('RuntimeError: ' + str(e.value)).startswith(str(g['full_image_error'][0]))


def test_root_finder_and_crossing_vs_stepwise_formulation(cuda):
    """psn_first_crossing against the torch formulation of rendering.py:457-504, and psn_root_find (all secant iterations
    in one launch, in-kernel positional encoding) against the step-by-step secant (one encoding + network + update launch
    per iteration on the compacted rays, the round-1 path): identical masks, depths equal bit for bit."""
    from psnerf_amd import hip
    from psnerf_amd.stage1.rendering import camera_origin, pixel_rays, sphere_intersection
    from psnerf_amd.synthetic import stage1_camera
    cfg, net, ren = _renderer(cuda)
    h, w = 48, 64
    K, c2w, S = stage1_camera(cfg, h=h, w=w)
    gen = torch.Generator().manual_seed(9)
    n = 333
    pix = torch.stack([torch.randint(0, w, (n,), generator=gen).float(), torch.randint(0, h, (n,), generator=gen).float()], -1)[None].to(cuda)
    cam = camera_origin(n, c2w.to(cuda))
    rays = pixel_rays(pix, K.to(cuda), c2w.to(cuda))
    rays = rays / rays.norm(2, 2).unsqueeze(-1)
    with torch.no_grad():
        st = ren._march_launch(cam, rays, 0.5, [256, 257], ren.depth_range, cfg['rendering']['radius'], False)
        # -- first crossing vs the reference's tensor formulation
        M = 256
        u = ren._u(M, cuda)
        p_prop = torch.empty(n, M, 3, device=cuda)
        far = sphere_intersection(cam[:, 0], rays, r=cfg['rendering']['radius'])[0][..., 1].contiguous()
        hip.sample_points(cam.reshape(-1, 3).contiguous(), rays.reshape(-1, 3).contiguous(), far.reshape(-1), p_prop, False,
                          float(ren.depth_range[0]), u)
        val = (ren._occ(p_prop.reshape(-1, 3)) - 0.5).view(1, n, M)
        from tests.ray_cases import first_crossing_reference   # the tensor formulation, shared with tests/test_ray_gpu.py
        mask_ref, first_free_ref, bracket_ref = first_crossing_reference(val[0], u[0], u[1], float(ren.depth_range[0]), far)
        flags = st['flags']
        assert torch.equal((flags & 1).bool(), mask_ref.reshape(-1)) and torch.equal((flags & 2).bool(), (val[0, :, 0] < 0))
        assert torch.equal(first_free_ref, val[0, :, 0] < 0)
        m = mask_ref.reshape(-1)
        for row, ref in enumerate(bracket_ref):
            assert torch.equal(st['bracket'][row][m], ref[m]), 'bracket row %d' % row
        # -- fused vs step-by-step secant
        d_fused = ren._march_finish(st, 8)
        d_step = ren._march_finish_compact(st, 8)
        # -- the feature-parallel root finder (16 rays per workgroup, output tiles split over the waves) vs the row-parallel
        #    engine: same arithmetic in the same order per output element, so the depths agree bit for bit
        import os
        os.environ['PSN_ROOT_FIND_ROW_PARALLEL'] = '1'
        try:
            d_rowpar = ren._march_finish(st, 8)
        finally:
            del os.environ['PSN_ROOT_FIND_ROW_PARALLEL']
    fin = torch.isfinite(d_step)
    assert torch.equal(fin, torch.isfinite(d_fused)) and int(m.sum()) > 20
    assert torch.equal(d_step == 0, d_fused == 0)
    # the same expressions in the same order, contraction off: bit for bit (measured by family H of tests/test_mlp_gpu.py, which
    # holds D[0] .. D[8] of both forms to the step-by-step composition on eleven networks)
    assert torch.equal(d_fused[fin], d_step[fin]), 'fused vs step-by-step secant: max |diff| = %g' % float((d_fused[fin] - d_step[fin]).abs().max())
    assert torch.equal(d_fused, d_rowpar), 'feature-parallel vs row-parallel root finder'


@pytest.mark.parametrize('n_steps,n', [(256, 333), (512, 200), (64, 70), (256, 4096)])
def test_march_sweep_with_early_exit_is_bit_identical(cuda, n_steps, n):
    """psn_march_sweep (sweep points generated + encoded in the occupancy kernel, one workgroup = 64 steps of one ray,
    blocks behind a ray's first sign change not evaluated) against the two-launch dense sweep (psn_sample_points on an
    [N, M, 3] tensor + psn_mlp_infer_pe): identical occupancies where both evaluate, and -- what the reference's result
    depends on, rendering.py:472-523 -- bit-identical brackets, masks and refined depths."""
    from psnerf_amd import hip
    from psnerf_amd.stage1.rendering import camera_origin, pixel_rays
    from psnerf_amd.synthetic import stage1_camera
    cfg, net, ren = _renderer(cuda)
    h, w = 48, 64
    K, c2w, S = stage1_camera(cfg, h=h, w=w)
    gen = torch.Generator().manual_seed(n_steps + n)
    pix = torch.stack([torch.randint(0, w, (n,), generator=gen).float(), torch.randint(0, h, (n,), generator=gen).float()], -1)[None].to(cuda)
    cam = camera_origin(n, c2w.to(cuda))
    rays = pixel_rays(pix, K.to(cuda), c2w.to(cuda))
    rays = rays / rays.norm(2, 2).unsqueeze(-1)
    args = (cam, rays, 0.5, [n_steps, n_steps + 1], ren.depth_range, cfg['rendering']['radius'], False)
    with torch.no_grad():
        ren.FUSED_SWEEP = False
        st_ref = ren._march_launch(*args)
        d_ref = ren._march_finish(st_ref, 8)
        ren.FUSED_SWEEP, ren.EARLY_EXIT = True, False
        st_dense = ren._march_launch(*args)
        ren.EARLY_EXIT = True
        st = ren._march_launch(*args)
        d = ren._march_finish(st, 8)
        # the occupancies themselves: the fused sweep without early exit == the two-launch sweep, bit for bit
        packed = net._occupancy_packed()
        u = ren._u(n_steps, cuda)
        far = st['far'].reshape(-1)
        occ_dense, _ = hip.march_sweep(packed.desc, packed.w, packed.b, cam.reshape(-1, 3).contiguous(), rays.reshape(-1, 3).contiguous(),
                                       far, u[0], u[1], float(ren.depth_range[0]), n_steps, 0.5, net.octaves_pe, 1.0 / net.rescale,
                                       early_exit=False)
        p_prop = torch.empty(n, n_steps, 3, device=cuda)
        hip.sample_points(cam.reshape(-1, 3).contiguous(), rays.reshape(-1, 3).contiguous(), far, p_prop, False, float(ren.depth_range[0]), u)
        occ_two = ren._occ(p_prop.reshape(-1, 3)).view(n, n_steps)
        occ_early, skip = hip.march_sweep(packed.desc, packed.w, packed.b, cam.reshape(-1, 3).contiguous(), rays.reshape(-1, 3).contiguous(),
                                          far, u[0], u[1], float(ren.depth_range[0]), n_steps, 0.5, net.octaves_pe, 1.0 / net.rescale,
                                          early_exit=True)
    assert torch.equal(occ_dense, occ_two)
    for key in ('bracket', 'flags'):
        assert torch.equal(st_ref[key], st_dense[key]) and torch.equal(st_ref[key], st[key]), key
    assert torch.equal(d_ref, d)
    hits = (st['flags'] & 1).bool()
    assert int(hits.sum()) > 10 and int((~hits).sum()) > 10
    # every value up to and including the pair of the first sign change equals the dense sweep; rays with a sign change (or
    # an occupied first point) raised their flag unless the change straddles two 64-step blocks
    val = occ_dense - 0.5
    neg = (val[:, :-1] * val[:, 1:]) < 0
    first = torch.where(neg.any(1), neg.float().argmax(1), torch.full((n,), n_steps - 2, device=cuda, dtype=torch.long))
    cols = torch.arange(n_steps, device=cuda)[None]
    needed = cols <= (first[:, None] + 1)
    needed &= (val[:, :1] < 0) | (cols < 64)  # a ray that starts inside the object is decided by its first block (rendering.py:522)
    assert torch.equal(occ_early[needed], occ_dense[needed])
    in_block = neg.any(1) & ((first % 64) != 63)
    assert bool((skip[in_block] != 0).all())
    # the flag records the LOWEST block that holds a sign change (INT_MAX - block): for a ray that starts in free space that
    # is the block of its first sign change, whatever order the workgroups ran in (a boolean let block b leave
    # when block b + 1 had raised it first)
    free_start = in_block & (val[:, 0] < 0)
    assert torch.equal((0x7fffffff - skip[free_start]).long(), first[free_start] // 64)
    if n_steps > 64:
        assert int((skip != 0).sum()) > 0


def test_shadow_ray_compaction_is_bit_identical(cuda):
    """light_visibility with in-box compaction (psn_shadow_points) == the dense formulation of rendering.py:378-408
    (every sample evaluated, out-of-box occupancies zeroed afterwards), bit for bit, incl. points outside the box."""
    from psnerf_amd import hip
    cfg, net, ren = _renderer(cuda)
    g = torch.Generator().manual_seed(2)
    surf = (torch.rand(300, 3, generator=g) * 2.4 - 1.2).to(cuda)  # some points outside the +-1.1 box
    ld = torch.nn.functional.normalize(torch.randn(7, 3, generator=g), dim=-1).to(cuda)
    with torch.no_grad():
        v = ren.light_visibility(surf=surf, light_dir=ld)
        n_in, n_all = ren.last_shadow_stats
        t = torch.linspace(0, 1, steps=128, device=cuda).view(1, 128, 1)
        d = 0.1 * (1.0 - t) + 3.5 * t
        p = surf[None, :, None, :] + ld[:, None, None, :] * d[None]
        alpha = ren._occ(p.reshape(-1, 3)).view(-1, 128)
        inside = torch.logical_and((p <= 1.1).all(dim=-1), (p >= -1.1).all(dim=-1)).view(-1, 128)
        assert n_in == int(inside.sum()) and 0 < n_in < n_all
        alpha = torch.where(inside, alpha, torch.zeros_like(alpha)).contiguous()
        ref = 1 - hip.composite_fwd(alpha, None, False, need_weights=False)[2]
    assert torch.equal(v, ref)
    # the host-synchronised form (launch sized by counter.item(), index_copy_ of the occupancies) gives the same bits; and a
    # scene with every sample outside the box (empty compacted list: every workgroup of the indirect launch leaves) is all lit
    ren.SHADOW_SYNC_FREE = False
    with torch.no_grad():
        assert torch.equal(ren.light_visibility(surf=surf, light_dir=ld), v)
        ren.SHADOW_SYNC_FREE = True
        far_away = surf * 0 + 5.0
        assert torch.equal(ren.light_visibility(surf=far_away, light_dir=ld), torch.ones_like(v))
        assert ren.last_shadow_stats[0] == 0


def test_indirect_occupancy_launch_reads_its_row_count_on_the_device(cuda):
    """psn_mlp_infer_pe_indirect: capacity-sized grid, device-resident length, scattered outputs -- equal to the direct launch
    on the valid prefix, untouched destinations elsewhere (lengths: 0, inside a workgroup, a workgroup boundary, full)."""
    cfg, net, ren = _renderer(cuda)
    g = torch.Generator().manual_seed(4)
    cap = 1000
    pts = (torch.rand(cap, 3, generator=g) * 2 - 1).to(cuda)
    perm = torch.randperm(3 * cap, generator=g)[:cap].to(cuda)
    packed = net._occupancy_packed()
    with torch.no_grad():
        ref = packed.on_points(pts, net.octaves_pe, 1.0 / net.rescale).reshape(-1)
        for n in (0, 1, 63, 64, 65, 640, cap):
            out = torch.full((3 * cap,), -7.0, device=cuda)
            cnt = torch.tensor([n], dtype=torch.int64, device=cuda)
            packed.on_points(pts, net.octaves_pe, 1.0 / net.rescale, out=out, n_rows_dev=cnt, out_rows=perm)
            want = torch.full((3 * cap,), -7.0, device=cuda)
            want[perm[:n]] = ref[:n]
            assert torch.equal(out, want), n
            dense = torch.full((cap,), -7.0, device=cuda)
            packed.on_points(pts, net.octaves_pe, 1.0 / net.rescale, out=dense, n_rows_dev=cnt)
            assert torch.equal(dense[:n], ref[:n]) and bool((dense[n:] == -7.0).all())


@pytest.mark.parametrize('n', [0, 1, 63, 64, 5000, 70001])
def test_occupancy_with_in_kernel_encoding_is_bit_identical(cuda, n):
    """psn_mlp_infer_pe (positional encoding formed in the kernel prologue, network.py:141-150 + 85-101 in one launch) ==
    psn_pe_encode + psn_mlp_launch on the [Q,64] table, bit for bit, incl. ragged row counts and far-away points."""
    from psnerf_amd import hip
    cfg, net, ren = _renderer(cuda)
    g = torch.Generator().manual_seed(n)
    p = ((torch.rand(n, 3, generator=g) - 0.5) * 6.0).to(cuda)
    if n > 2:
        p[0] = 0.0
        p[1] = torch.tensor([250.0, -1e-3, 3.1415927], device=cuda)  # large sin / cos arguments (2^5 * 250 / rescale)
    net = net.to(cuda)
    with torch.no_grad():
        packed = net._occupancy_packed()
        got = net.occupancy(p)
        if n == 0:
            assert got.shape == (0, 1)
            return
        tab = hip.pe_encode(p, net.octaves_pe, 64, 1.0 / net.rescale)
        ref = packed(tab, n)
    assert got.shape == ref.shape == (n, 1)
    assert torch.equal(got, ref)


def test_render_and_gradient_matches_the_two_separate_calls(cuda):
    """NeuralNetwork.render_and_gradient (surface-normal points riding behind the render samples through ONE set of
    geometry-network launches, features / d features for the render rows only) == forward(..., return_addocc=True) +
    gradient(extra): identical values (same arithmetic per row), parameter gradients equal to summation order."""
    from psnerf_amd.stage1 import NeuralNetwork
    cfg = stage1_cfg('bear')
    g = torch.Generator().manual_seed(3)
    p = ((torch.rand(37, 24, 3, generator=g) - 0.5) * 1.6).to(cuda)
    view = torch.nn.functional.normalize(torch.randn(37, 24, 3, generator=g), dim=-1).to(cuda)
    extra = ((torch.rand(2 * 37, 3, generator=g) - 0.5) * 1.6).to(cuda)
    wr, wo, wg = torch.randn(37, 24, 3, generator=g).to(cuda), torch.randn(37, 24, 1, generator=g).to(cuda), torch.randn(74, 1, 3, generator=g).to(cuda)
    res = []
    for merged in (False, True):
        net = NeuralNetwork(cfg)
        net.load_state_dict(stage1_state_dict(cfg, seed=5))
        net = net.to(cuda)
        if merged:
            rgb, occ, gr = net.render_and_gradient(p, view, extra)
        else:
            rgb, occ = net(p, view, return_addocc=True)
            gr = net.gradient(extra)
        ((rgb * wr).sum() + (occ * wo).sum() + (gr * wg).sum() * 1e-2).backward()
        res.append((rgb.detach(), occ.detach(), gr.detach(), {k: q.grad.clone() for k, q in net.named_parameters() if q.grad is not None}))
    (rgb0, occ0, g0, pg0), (rgb1, occ1, g1, pg1) = res
    assert g1.shape == (74, 1, 3)
    assert torch.equal(rgb0, rgb1) and torch.equal(occ0, occ1) and torch.equal(g0, g1)
    assert pg0.keys() == pg1.keys() and len(pg0) > 20
    for k in pg0:
        assert_close(pg1[k].cpu(), pg0[k].cpu(), 2e-5, 'd ' + k)  # max-normalised: gradient tensors


def test_fused_optimizer_does_not_leave_stale_weight_packs(cuda):
    """torch.optim.Adam(fused=True) updates the parameters WITHOUT bumping their version counters, on which the weight-pack
    caches are keyed: the trainer invalidates the packs after every optimiser step, so three steps with the fused
    implementation follow the foreach implementation (same update rule; last-bit differences of the fused arithmetic only)."""
    from psnerf_amd.stage1 import NeuralNetwork, Renderer, Trainer
    from psnerf_amd.synthetic import stage1_batch
    cfg = stage1_cfg('bunny', **{'training.n_training_points': 256})
    batch = {k: v.to(cuda) for k, v in stage1_batch(cfg, h=48, w=64, seed=1).items()}
    g = torch.Generator().manual_seed(4)
    pix = torch.stack([torch.randint(0, 64, (256,), generator=g).float(), torch.randint(0, 48, (256,), generator=g).float()], -1)[None]
    losses = {}
    for fused in (False, True):
        net = NeuralNetwork(cfg)
        net.load_state_dict(stage1_state_dict(cfg, seed=5))
        torch.manual_seed(0)
        tr = Trainer(Renderer(net, cfg, device=cuda), torch.optim.Adam(net.parameters(), lr=1e-3, fused=fused), cfg, device=cuda)
        losses[fused] = []
        for it in range(3):
            torch.manual_seed(100 + it)
            losses[fused].append(float(tr.train_step(batch, it=6000, pix=pix.clone())['loss'].detach()))
    assert losses[False][0] == losses[True][0]
    assert losses[False][2] != losses[False][0], 'the steps must move the loss for this test to mean anything'
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) <= 1e-4 * abs(a), (losses[False], losses[True])


# ---- split-bf16 ("bf16x6") occupancy engine: opt-in, gradient-free queries only (csrc/mlp_infer_x3.hip, OCC variant) -----------
@pytest.mark.parametrize('n', [1, 127, 128, 129, 5000, 70001])
def test_x3_occupancy_engine_has_fp32_class_accuracy(cuda, n):
    """NeuralNetwork.occupancy with inference_precision = 'bf16x6' (every fp32 operand as three bf16 planes, six partial
    products per multiply, softplus in fp32, encoding formed in the kernel) against the float64 evaluation of the oracle:
    the SAME elementwise gate the exact engine has to pass (1e-4 |ref| + 1e-6), and an error of the size of the exact-fp32
    engine's own; ragged row counts, far-away points with large sin / cos arguments."""
    from oracle import stage1 as o1
    cfg, net, ren = _renderer(cuda)
    g = torch.Generator().manual_seed(n)
    p = ((torch.rand(n, 3, generator=g) - 0.5) * 2.6)
    if n > 2:
        p[0] = 0.0
        p[1] = torch.tensor([250.0, -1e-3, 3.1415927])
    onet = o1.NeuralNetwork(cfg)
    onet.load_state_dict(stage1_state_dict(cfg, seed=11))
    onet.double()
    with torch.no_grad():
        truth = onet(p.double(), only_occupancy=True).reshape(-1, 1)
        assert net.inference_precision == 'fp32'
        exact = net.occupancy(p.to(cuda)).cpu()
        net.inference_precision = 'bf16x6'
        got = net.occupancy(p.to(cuda)).cpu()
        net.inference_precision = 'fp32'
    assert got.shape == (n, 1)
    assert_close(got, truth.float(), 1e-4, 'bf16x6 occupancy vs float64', atol=ATOL_UNIT)
    e_x3, e_32 = float((got.double() - truth).abs().max()), float((exact.double() - truth).abs().max())
    assert e_x3 <= 3.0 * e_32 + 2e-7, (e_x3, e_32)


def test_x3_occupancy_indirect_form_and_gradient_paths_stay_exact(cuda):
    """The indirect form (capacity-sized grid, device-resident length, scattered outputs: the shadow-ray path) equals the
    direct launch on the valid prefix and leaves other destinations alone; with gradients enabled the module ignores the
    opt-in (training never runs on the split engine)."""
    cfg, net, ren = _renderer(cuda)
    g = torch.Generator().manual_seed(4)
    cap = 1000
    pts = (torch.rand(cap, 3, generator=g) * 2 - 1).to(cuda)
    perm = torch.randperm(3 * cap, generator=g)[:cap].to(cuda)
    net.inference_precision = 'bf16x6'
    try:
        with torch.no_grad():
            packed = net._occupancy_packed(allow_x3=True)
            assert type(packed).__name__ == 'PackedX3Occ'
            ref = packed.on_points(pts, net.octaves_pe, 1.0 / net.rescale).reshape(-1)
            for n in (0, 1, 127, 128, 129, 640, cap):
                out = torch.full((3 * cap,), -7.0, device=cuda)
                cnt = torch.tensor([n], dtype=torch.int64, device=cuda)
                packed.on_points(pts, net.octaves_pe, 1.0 / net.rescale, out=out, n_rows_dev=cnt, out_rows=perm)
                want = torch.full((3 * cap,), -7.0, device=cuda)
                want[perm[:n]] = ref[:n]
                assert torch.equal(out, want), n
        assert type(net._occupancy_packed(allow_x3=True)).__name__ == 'PackedMLP'  # gradients enabled: the exact engine
        assert type(net._occupancy_packed()).__name__ == 'PackedMLP'               # march sweep / root finder: always exact
    finally:
        net.inference_precision = 'fp32'


@pytest.mark.parametrize('n_steps,n', [(256, 333), (512, 200), (128, 70), (256, 4096)])
def test_x3_march_sweep_equals_the_two_launch_form_and_exits_early(cuda, n_steps, n):
    """psn_march_sweep_x3 (the sweep of rendering.py:447-462 on the split-bf16 engine: points formed and encoded in the kernel, a
    workgroup = 128 steps of one ray, blocks behind a ray's first sign change not evaluated) against the two-launch form on the SAME
    engine (psn_sample_points + psn_mlp_infer_x3_occ): identical occupancies where both evaluate, identical brackets / masks /
    refined depths; the flag records the lowest block with a sign change."""
    from psnerf_amd import hip
    from psnerf_amd.stage1.rendering import camera_origin, pixel_rays
    from psnerf_amd.synthetic import stage1_camera
    cfg, net, ren = _renderer(cuda)
    net.inference_precision = 'bf16x6'
    try:
        h, w = 48, 64
        K, c2w, S = stage1_camera(cfg, h=h, w=w)
        gen = torch.Generator().manual_seed(n_steps + n)
        pix = torch.stack([torch.randint(0, w, (n,), generator=gen).float(), torch.randint(0, h, (n,), generator=gen).float()], -1)[None].to(cuda)
        cam = camera_origin(n, c2w.to(cuda))
        rays = pixel_rays(pix, K.to(cuda), c2w.to(cuda))
        rays = rays / rays.norm(2, 2).unsqueeze(-1)
        args = (cam, rays, 0.5, [n_steps, n_steps + 1], ren.depth_range, cfg['rendering']['radius'], False)
        with torch.no_grad():
            ren.FUSED_SWEEP = False
            st_ref = ren._march_launch(*args)  # sample_points + the x3 engine on the point tensor
            d_ref = ren._march_finish(st_ref, 8)
            ren.FUSED_SWEEP, ren.EARLY_EXIT = True, False
            st_dense = ren._march_launch(*args)
            ren.EARLY_EXIT = True
            st = ren._march_launch(*args)
            d = ren._march_finish(st, 8)
            pk = net._occupancy_packed_x3()
            u = ren._u(n_steps, cuda)
            far = st['far'].reshape(-1)
            o3, d3 = cam.reshape(-1, 3).contiguous(), rays.reshape(-1, 3).contiguous()
            occ_dense, _ = pk.march_sweep(o3, d3, far, u[0], u[1], float(ren.depth_range[0]), n_steps, 0.5, net.octaves_pe, 1.0 / net.rescale, early_exit=False)
            p_prop = torch.empty(n, n_steps, 3, device=cuda)
            hip.sample_points(o3, d3, far, p_prop, False, float(ren.depth_range[0]), u)
            occ_two = pk.on_points(p_prop.reshape(-1, 3), net.octaves_pe, 1.0 / net.rescale).view(n, n_steps)
            occ_early, skip = pk.march_sweep(o3, d3, far, u[0], u[1], float(ren.depth_range[0]), n_steps, 0.5, net.octaves_pe, 1.0 / net.rescale, early_exit=True)
    finally:
        ren.FUSED_SWEEP = ren.EARLY_EXIT = True
        net.inference_precision = 'fp32'
    assert torch.equal(occ_dense, occ_two)
    for key in ('bracket', 'flags'):
        assert torch.equal(st_ref[key], st_dense[key]) and torch.equal(st_ref[key], st[key]), key
    assert torch.equal(d_ref, d)
    hits = (st['flags'] & 1).bool()
    assert int(hits.sum()) > 10 and int((~hits).sum()) > 10
    val = occ_dense - 0.5
    neg = (val[:, :-1] * val[:, 1:]) < 0
    first = torch.where(neg.any(1), neg.float().argmax(1), torch.full((n,), n_steps - 2, device=cuda, dtype=torch.long))
    cols = torch.arange(n_steps, device=cuda)[None]
    needed = cols <= (first[:, None] + 1)
    needed &= (val[:, :1] < 0) | (cols < 128)
    assert torch.equal(occ_early[needed], occ_dense[needed])
    in_block = neg.any(1) & ((first % 128) != 127)
    assert bool((skip[in_block] != 0).all())
    free_start = in_block & (val[:, 0] < 0)
    assert torch.equal((0x7fffffff - skip[free_start]).long(), first[free_start] // 128)
    if n_steps > 128:
        assert int((skip != 0).sum()) > 0


def test_x3_occupancy_engine_passes_the_march_and_light_visibility_goldens(cuda):
    """Gates of the opt-in engine: with inference_precision = 'bf16x6' the ray march of the golden case
    classifies every ray as the reference does (hit / miss / starts-inside masks EQUAL), the refined depths and the
    shadow-ray light visibility stay within the bounds the exact path is held to."""
    from psnerf_amd.stage1.rendering import camera_origin, pixel_rays
    g = np.load(os.path.join(GOLDEN, 'stage1_march.npz'))
    cfg, net, ren = _renderer(cuda)
    net.inference_precision = 'bf16x6'
    try:
        pix, K, c2w = T(g['pix'], cuda), T(g['K'], cuda), T(g['c2w'], cuda)
        cam = camera_origin(pix.shape[1], c2w)
        rays = pixel_rays(pix, K, c2w)
        rays = rays / rays.norm(2, 2).unsqueeze(-1)
        d = ren.ray_marching(cam, rays, n_steps=[256, 257], n_secant_steps=8, rad=2.0, depth_range=[2, 6]).cpu()
        ref = torch.from_numpy(g['d_i'])
        fin = torch.isfinite(ref)
        assert torch.equal(fin, torch.isfinite(d)), 'hit / miss classification differs'
        assert torch.equal(ref == 0, d == 0)
        assert_close(d[fin], ref[fin], 1e-4, 'd_i', atol=ATOL_DEPTH)
        lv = ren.light_visibility(surf=T(g['surf'], cuda), light_dir=T(g['ldir'], cuda)).cpu()
        assert_close(lv, g['light_vis'], 1e-4, 'light visibility', atol=ATOL_UNIT)
    finally:
        net.inference_precision = 'fp32'


def test_invalidate_packs_after_data_edit_stage1(cuda):
    """The stage-1 counterpart of test_stage2_gpu.test_invalidate_packs_after_data_edit: every weight pack of NeuralNetwork
    (occupancy, geometry / appearance chains, negated logit) is cached by parameter version + storage address; an edit through
    ``.data`` changes neither, so callers announce it with invalidate_packs(); load_state_dict invalidates by itself.  Unchanged
    parameters: a second call runs on the cached packs and is bit-identical.
    "Changed" = max |difference| > 1e-4: the edits scale a hidden layer's weight_g by 1.5 / 0.5 (an O(1) change of every
    output; weight_v would not do, w = g v / |v| is invariant to its scale), fp32 rounding is ~1e-6."""
    from psnerf_amd.stage1 import NeuralNetwork
    g = np.load(os.path.join(GOLDEN, 'stage1_net_h256.npz'))
    cfg = stage1_cfg('bunny')
    net = NeuralNetwork(cfg)
    net.load_state_dict(stage1_state_dict(cfg, seed=11))
    net.to(cuda)
    p, ray_d = T(g['p'], cuda), T(g['ray_d'], cuda)
    flat = p.reshape(-1, 3).contiguous()

    def run():
        with torch.no_grad():
            occ = net.occupancy(flat).clone()
            logit = net._logit_packed().on_points(flat, net.octaves_pe, 1.0 / net.rescale).clone()
        rgb = net(p.clone(), ray_d).detach().clone()  # (with a graph: the fused geometry / appearance chains)
        return {'occupancy': occ, 'render': rgb, 'logit': logit}

    def assert_same(x, y):
        for k in x:
            assert torch.equal(x[k], y[k]), k

    def assert_changed(x, y):
        for k in x:
            d = float((x[k] - y[k]).abs().max())
            print('%s: max |difference| %.3e' % (k, d))
            assert d > 1e-4, k

    a = run()
    assert_same(a, run())
    net.lin2.weight_g.data.mul_(1.5)  # no version bump
    net.invalidate_packs()
    b = run()
    assert_changed(a, b)
    assert_same(b, run())
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    sd['lin3.weight_g'] = sd['lin3.weight_g'] * 0.5
    net.load_state_dict(sd)
    c = run()
    assert_changed(b, c)
    assert_same(c, run())
