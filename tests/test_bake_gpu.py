"""The texture bake on the GPU (csrc/meshbake.hip through psnerf_amd/hip.py and psnerf_amd/meshbake.py) against the numpy definition in
the same module.  Outputs land in guarded buffers (NaN / 0xFF), so a row or texel the kernel skips -- or one it should not have touched
-- shows.

Gates, with where they come from:
  psn_atlas_points / scatter / fill / sample   EQUAL, bit for bit (NaN compared by bytes): the layout is integer arithmetic, the kernels do
              the definition's float64 operations in the definition's order with contraction off, and division, square root, floor and
              the float32 conversions are correctly rounded on both sides.
  bake        the chunked bake against ONE direct call of the same networks on all rows: equal bit for bit -- renderer.py relies on the
              fused engines being row-wise independent of what else is in the launch; albedo within 1e-4 of the oracle's network (the
              project's output gate).
  round trip  2^-23 max|f| (one float32 rounding per texel, kept by the convex combination) plus the caster's own point error
              |t| 2^-52 |d|.
"""
import numpy as np
import pytest
import torch

from tests import bake_cases as bc
from psnerf_amd import meshbake as mb

pytestmark = pytest.mark.gpu
CHANNELS = (1, 3, 9, 27)


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)


def same_bits(t, a):
    """A device tensor and a numpy array of the same dtype hold the same bytes (NaN-safe, -0.0 is not +0.0)."""
    a = np.ascontiguousarray(a)
    h = t.cpu().numpy()
    return h.dtype == a.dtype and h.shape == a.shape and np.array_equal(h.view(np.uint8), a.view(np.uint8))


def cases():
    """(name, T) for every mesh and size that fit; what does not fit raises on the host already (tests/test_bake_cpu.py)."""
    return [(name, T) for name, (v, f, vn) in bc.meshes().items() for T in bc.SIZES if bc.fits(T, len(f))[0]]


@pytest.mark.parametrize('name', list(bc.meshes()))
def test_points_equal_the_definition_bit_for_bit(cuda, name):
    """Every size that fits x face ranges that start and end mid-cell, with the mesh's vertex normals and without."""
    from psnerf_amd import hip
    v, f, vn = bc.meshes()[name]
    d_v, d_f, d_vn = dev(v, cuda), dev(f, cuda), dev(vn, cuda)
    n = 0
    for T in [T for nm, T in cases() if nm == name]:
        a = mb.Atlas(T, len(f))
        for normals, d_normals in ((vn, d_vn), (None, None)) if vn is not None else ((None, None),):
            whole = mb.host_atlas_points(a, v, f, normals)
            for f0, f1 in bc.face_ranges(len(f)):
                R = (f1 - f0) * a.K
                guard = (torch.full((R, 3), float('nan'), dtype=torch.float64, device=cuda), torch.full((R, 3), float('nan'), dtype=torch.float32, device=cuda),
                         torch.full((R, 3), float('nan'), dtype=torch.float64, device=cuda))
                out = hip.atlas_points(d_v, d_f, d_normals, T, a.c, f0, f1, out=guard)
                for what, t, h in zip(('points', 'points_f32', 'normals'), out, whole):
                    h = h[f0 * a.K:f1 * a.K]
                    assert same_bits(t, h), '%s, T = %d, faces [%d, %d): %s differs in %d of %d elements' % (
                        name, T, f0, f1, what, int((t.cpu().numpy() != h).sum()), h.size)
                n += 1
            d = mb.atlas_points(a, d_v, d_f, d_normals)                    # the dispatch, fresh outputs
            assert all(same_bits(t, h) for t, h in zip(d, whole))
    assert n >= 2
    with pytest.raises(RuntimeError):
        hip.atlas_points(d_v, d_f, None, 8, 3)
    with pytest.raises(RuntimeError):
        hip.atlas_points(d_v, d_f, None, 16, 16 if len(f) > 2 else 32)     # the faces do not fit (or the cell exceeds T): PSN_E_ARG


@pytest.mark.parametrize('name', list(bc.meshes()))
def test_scatter_and_fill_equal_the_definition_bit_for_bit(cuda, name):
    """float and uint8 textures, C in 1, 3, 9, 27, every size that fits, face ranges that start and end mid-cell; the texture starts as
    a guard pattern on both sides, so the comparison of the WHOLE texture also shows that nothing outside the range is written and that
    the fill touches the unowned texels only."""
    from psnerf_amd import hip
    F = len(bc.meshes()[name][1])
    for T in [T for nm, T in cases() if nm == name]:
        a = mb.Atlas(T, F)
        for ci, C in enumerate(CHANNELS):
            all_rows = bc.rows_for(F * a.K, C, seed=T + C)
            for ri, (f0, f1) in enumerate(bc.face_ranges(F)):
                rows = np.ascontiguousarray(all_rows[f0 * a.K:f1 * a.K])
                for u8 in (False, True):
                    guard = np.full((T, T, C), 0xEE, dtype=np.uint8) if u8 else np.full((T, T, C), np.nan, dtype=np.float32)
                    fill = (None, 0.25, -3.0)[(ci + ri + u8) % 3]
                    want = mb.host_atlas_scatter(a, rows, f0, f1, out=guard.copy(), fill=fill)
                    got = mb.atlas_scatter(a, dev(rows, cuda), f0, f1, out=dev(guard, cuda), fill=fill)
                    assert same_bits(got, want), '%s, T = %d, C = %d, faces [%d, %d), %s: %d texel elements differ' % (
                        name, T, C, f0, f1, 'uint8' if u8 else 'float32', int((got.cpu().numpy().view(np.uint8) != want.view(np.uint8)).sum()))
            fresh = mb.atlas_scatter(a, dev(all_rows, cuda), fill=0.5, u8=bool(ci % 2))
            assert same_bits(fresh, mb.host_atlas_scatter(a, all_rows, fill=0.5, u8=bool(ci % 2)))
    tex = torch.zeros(16, 16, 3, device=cuda)
    with pytest.raises(RuntimeError):
        hip.atlas_scatter(torch.zeros(5, 3, device=cuda), tex, 4, 2)      # 2 faces x 6 rows expected
    with pytest.raises(RuntimeError):
        hip.atlas_scatter(torch.zeros(240, 3, device=cuda), tex, 4, 40)   # 40 faces do not fit 4 x 4 cells: PSN_E_ARG


@pytest.mark.parametrize('Q', [1, 63, 64, 65, 4097])
def test_sample_equals_the_definition_bit_for_bit(cuda, Q):
    """Every mesh and size x C in 1, 3, 9, 27 (one C per case, all four over the cases): corners, edge midpoints, hypotenuse and
    interior points, faces in the last cell of a cell row and of the atlas, misses (-1), faces beyond F, NaN barycentrics."""
    n_miss = 0
    for i, (name, T) in enumerate(cases()):
        F = len(bc.meshes()[name][1])
        a = mb.Atlas(T, F)
        C = CHANNELS[(i + Q) % 4]
        g = np.random.RandomState(i)
        tex = (g.standard_normal((T, T, C)) * 3).astype(np.float32)
        face, bary = bc.queries(a, Q, seed=i + Q)
        if Q >= 64:
            bary[7] = [0.2, np.inf, 0.1]                                   # a position that is not finite
            bary[15] = [-40.0, 20.5, 20.5]                                 # far outside the texture: clamped
        want = mb.host_atlas_sample(a, face, bary, tex)
        out = torch.full((Q, C), 7.0, dtype=torch.float64, device=cuda)
        from psnerf_amd import hip
        got = hip.atlas_sample(dev(face, cuda), dev(bary, cuda), dev(tex, cuda), a.c, F, out=out)
        assert same_bits(got, want), '%s, T = %d, C = %d: %d of %d rows differ' % (
            name, T, C, int((got.cpu().numpy().view(np.uint64) != want.view(np.uint64)).any(1).sum()), Q)
        assert same_bits(mb.atlas_sample(a, dev(face, cuda), dev(bary, cuda), dev(tex, cuda)), want)
        n_miss += int(np.isnan(want).all(1).sum())
    assert Q < 8 or n_miss > 0


def test_chunks_compose(cuda):
    """A bake in three ragged face ranges (27 + 27 + 25 of 79 faces, so cells are split between chunks) gives the bytes of one range."""
    a = mb.Atlas(64, 79)
    for C, u8 in ((3, False), (27, False), (3, True)):
        rows = bc.rows_for(79 * a.K, C, seed=C)
        d_rows = dev(rows, cuda)
        whole = mb.atlas_scatter(a, d_rows, fill=0.25, u8=u8)
        tex = torch.full((64, 64, C), 0xEE if u8 else float('nan'), dtype=torch.uint8 if u8 else torch.float32, device=cuda)
        for n, (f0, f1) in enumerate(((0, 27), (27, 54), (54, 79))):
            mb.atlas_scatter(a, d_rows[f0 * a.K:f1 * a.K], f0, f1, out=tex, fill=0.25 if n == 0 else None)
        assert same_bits(tex, whole.cpu().numpy()) and same_bits(whole, mb.host_atlas_scatter(a, rows, fill=0.25, u8=u8))


@pytest.mark.parametrize('case', list(bc.MODEL_CASES))
def test_bake_materials_on_the_device(cuda, case):
    """tests/test_bake_cpu.py::test_bake_materials_on_the_host on the device, under ops.STRICT (the fused engines or an error): every
    owned texel equals, bit for bit, ONE direct call of the same networks on all rows; unowned texels hold the fill; the albedo is
    within 1e-4 of the oracle's network."""
    from oracle import stage2 as o2
    from psnerf_amd import ops
    net, onet = bc.make_models(case)
    net.to(cuda)
    v, f, vn = bc.meshes()['icosphere(1)']
    ops.reset_hits()
    with ops.strict():
        baked = mb.bake_materials(net, (v, f, vn), size=64, chunk_faces=27, fill=-2.0)
        a = baked['atlas']
        p, p32, nrm = mb.atlas_points(a, dev(v, cuda), dev(f, cuda), dev(vn, cuda))
        with torch.no_grad():
            net.eval()
            cols = net._cols(net.n_freqs, cuda)
            pe = net._pe(p32, net.n_freqs)
            direct = {'albedo': net.albedo_net(pe, cols), 'specular': net.rough_net(pe, cols)}
            if 'sgbasis' in case:
                direct['specular'] = torch.relu(direct['specular'])
            direct['normal'] = (ops.normalize_rows(net.normal_net(net._pe(p32, net.n_freqs_n), net._cols(net.n_freqs_n, cuda)))
                                if 'normal net' in case else nrm.float())
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    assert ops.HITS.get('FusedReluNet', 0) >= 2 * (3 + 1)                  # the engines ran: 3 chunks + the direct call, two networks at least
    assert (a.T, a.F) == (64, 80) and all(baked[k].is_cuda and baked[k].dtype == torch.float32 for k in mb.MAPS)
    assert baked['specular'].shape == (64, 64, 27 if 'sgbasis' in case else 1)
    assert same_bits(p32, mb.host_atlas_points(a, v, f, vn)[1])
    xs, ys = a.texels()
    free = a.owner()[0] < 0
    for k in mb.MAPS:
        got, want = baked[k].cpu().numpy(), direct[k].cpu().numpy()
        dist = np.abs(got[ys, xs] - want).max()
        print('%s, %s: max |chunked bake - one direct call| = %g' % (case, k, dist))
        assert np.array_equal(got[ys, xs].view(np.uint32), want.view(np.uint32)), '%s: %g' % (k, dist)
        assert (got[free] == -2.0).all()
    with torch.no_grad():
        oracle_albedo = onet.albedo_net(o2.embed(p32.cpu(), 10)).numpy()
    err = np.abs(baked['albedo'].cpu().numpy()[ys, xs] - oracle_albedo).max()
    print('%s: max |albedo - oracle| = %g' % (case, err))
    assert err < 1e-4, err


def test_round_trip_through_the_caster(cuda):
    """render_view of icosphere(2) at 32 x 40 with textures= of a baked affine field, on the device: every hit pixel's value is within
    2^-23 max|f| (+ the caster's point error |t| 2^-52 |d|) of the field at out['points']; misses are NaN; without textures the dict
    has exactly today's keys and the same values."""
    from psnerf_amd import meshrender as mr, ops
    v, f, _ = bc.meshes()['icosphere(2)']
    a = mb.Atlas(256, len(f))
    tex, top = bc.bake_affine(a, v, f)
    d_tex = mb.atlas_scatter(a, dev(bc.affine(mb.host_atlas_points(a, v, f)[0]).astype(np.float32), cuda))
    assert same_bits(d_tex, tex)
    H, W = 32, 40
    K, c2w = bc.view(H, W)
    with ops.strict():
        plain = mr.render_view((v, f), K, c2w, H, W, device=cuda)
        out = mr.render_view((v, f), K, c2w, H, W, device=cuda, textures={'field': d_tex}, atlas=a)
    assert sorted(plain) == ['depth', 'mask', 'normals', 'points', 't', 'tri'] and sorted(out) == sorted(list(plain) + ['field'])
    assert all(x.is_cuda for x in out.values()) and all(torch.equal(plain[k], out[k]) for k in plain)
    mask = out['mask'].cpu().numpy()
    got = out['field'].cpu().numpy()
    assert got.shape == (H, W, 4) and got.dtype == np.float64 and 100 < mask.sum() < H * W and np.isnan(got[~mask]).all()
    want = bc.affine(out['points'].cpu().numpy()[mask])
    slack = 2.0 ** -23 * top + out['depth'].cpu().numpy()[mask] * 2.0 ** -52
    err = np.abs(got[mask] - want).max(axis=-1)
    assert (err <= slack).all(), '%d of %d hit pixels, the worst by %g (allowed %g)' % (int((err > slack).sum()), len(err), err.max(), slack.min())
    host = mr.render_view((v, f), K, c2w, H, W, textures={'field': tex}, atlas=a)      # the host path of the same call: the same lookups
    same = mask & host['mask'].numpy() & (out['tri'].cpu().numpy() == host['tri'].numpy())
    assert same.sum() > 0.9 * mask.sum() and np.abs(got[same] - host['field'].numpy()[same]).max() <= 2.0 ** -23 * top
