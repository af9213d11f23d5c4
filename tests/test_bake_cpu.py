"""The texture bake on the host: psnerf_amd/meshbake.py's numpy functions, which are the definition the kernels are held to
(tests/test_bake_gpu.py).  The layout is checked as integers, from the texel's side (an inverse written here) against the face's side (the
module's forward map); the lookups against faces numbered one by one and against an affine field; the bytes against the to_img
expression; the writer by reading its files back; the bake against a direct, unchunked evaluation of the same networks and against the
oracle's network.

Gates, with where they come from:
  isolation   4 x 2^-53 relative: the four texels read hold the same float32 number, and (1 - fy)((1 - fx) t + fx t) + fy (...) rounds
              at most four times around it.
  affine      2^-23 max|f|: one float32 rounding per texel (2^-24 relative), kept by the convex combination of the lookup, plus the
              float64 roundings of the points, the lookup and the test's own evaluation of the field, which are far below the other half.
  bake        chunked against unchunked on the CPU: the same float32 layers on other row counts, where the BLAS may block its dot
              products (at most 191 terms, outputs of order 1) differently: 1e-5, a tenth of the project's output gate against the
              oracle, which is the 1e-4 the albedo is then held to.
"""
import os

import numpy as np
import pytest
import torch

from tests import bake_cases as bc
from psnerf_amd import meshbake as mb


def inverse_layout(T, F, c):
    """The layout from the texel's side, straight from the statement of the atlas: per texel [y, x] the owning face (-1: none) and k."""
    G, n = T // c, c - 3
    y, x = np.meshgrid(np.arange(T), np.arange(T), indexing='ij')
    cx, cy = x // c, y // c
    i, j = x - cx * c, y - cy * c
    second = i + j > c - 1
    i, j = np.where(second, c - 1 - i, i), np.where(second, c - 1 - j, j)
    face = 2 * (cy * G + cx) + second
    free = (cx >= G) | (cy >= G) | ((x - cx * c) + (y - cy * c) == c - 1) | (face >= F)
    k = j * (n + 2) - j * (j - 1) // 2 + i
    return np.where(free, -1, face), np.where(free, -1, k)


@pytest.mark.parametrize('T', [16, 17, 64, 250])
def test_atlas_integers(T):
    """c is maximal; every owned texel has exactly one (f, k); k runs 0 .. K - 1 without gaps per face; no two faces share a texel; the
    unowned texels are exactly the diagonals, the free half of the last cell, the free cells and the margin; c < 4 raises and names F
    and the smallest T that would do."""
    seen = 0
    for F in (1, 2, 3, 7, 8, 9, 31, 32, 33, 80):
        cells = (F + 1) // 2
        for cell in (None, 4, 5, 8):
            feasible = [c for c in range(1, T + 1) if (T // c) ** 2 >= cells]
            c_max = max(feasible) if feasible else 0
            ok = c_max >= 4 if cell is None else (cell in feasible)
            if not ok:
                with pytest.raises(ValueError) as e:
                    mb.Atlas(T, F, cell)
                need = 4 * min(g for g in range(1, F + 2) if g * g >= cells)
                assert 'F = %d' % F in str(e.value) and 'T >= %d' % need in str(e.value)
                if cell is None:
                    assert need > T and (need // 4) ** 2 >= cells       # ... and that T would do, one less would not
                    mb.Atlas(need, F)
                    with pytest.raises(ValueError):
                        mb.Atlas(need - 1, F)
                continue
            a = mb.Atlas(T, F, cell)
            c = c_max if cell is None else cell
            assert (a.T, a.F, a.c, a.G, a.n, a.K) == (T, F, c, T // c, c - 3, (c - 1) * c // 2)
            face, k = inverse_layout(T, F, c)
            own_f, own_k = a.owner()
            assert np.array_equal(own_f, face) and np.array_equal(own_k, k)
            x, y = a.texels()
            assert x.shape == (F * a.K,) and x.min() >= 0 and y.min() >= 0 and x.max() < T and y.max() < T
            assert len(np.unique(y * T + x)) == F * a.K                                  # no texel twice: no two (f, k) share one
            assert np.array_equal(face[y, x], np.repeat(np.arange(F), a.K))               # the forward map lands in its own face ...
            assert np.array_equal(k[y, x], np.tile(np.arange(a.K), F))                    # ... at its own k: 0 .. K - 1, no gaps
            assert int((face >= 0).sum()) == F * a.K                                      # and nothing else is owned
            i, j = a.local()
            assert np.array_equal(j * (a.n + 2) - j * (j - 1) // 2 + i, np.arange(a.K)) and (i + j).max() == a.n + 1 and i.min() == 0
            cr = a.corners()
            q = np.arange(F) // 2
            X0, Y0 = (q % a.G) * c, (q // a.G) * c
            h = np.arange(F) % 2
            want = np.where(h[:, None, None] == 0, np.stack([np.stack([X0, Y0], -1), np.stack([X0 + a.n, Y0], -1), np.stack([X0, Y0 + a.n], -1)], 1),
                            np.stack([np.stack([X0 + c - 1, Y0 + c - 1], -1), np.stack([X0 + c - 1 - a.n, Y0 + c - 1], -1),
                                      np.stack([X0 + c - 1, Y0 + c - 1 - a.n], -1)], 1))
            assert np.array_equal(cr, want)
            uv = mb.atlas_uv(a)
            assert np.array_equal(uv[..., 0], (cr[..., 0] + 0.5) / T) and np.array_equal(uv[..., 1], 1.0 - (cr[..., 1] + 0.5) / T)
            seen += 1
    assert seen >= (4 if T < 64 else 30)
    with pytest.raises(ValueError):
        mb.Atlas(T, 0)


def fitting(name):
    v, f, vn = bc.meshes()[name]
    return [T for T in bc.SIZES if bc.fits(T, len(f))[0]], v, f, vn


@pytest.mark.parametrize('name', list(bc.meshes()))
def test_faces_are_isolated(name):
    """Rows whose value is the face number, scattered, then looked up at every face's corners and edge midpoints and at random interior,
    leg and hypotenuse points: the face's own number comes back.  A wrong gutter or a wrong barycentric order reads a neighbour's
    texel (or the fill, -1000) and shows; a miss and a face beyond F give NaN."""
    sizes, v, f, _ = fitting(name)
    F = len(f)
    for T in [T for T in bc.SIZES if T not in sizes]:
        with pytest.raises(ValueError):
            mb.Atlas(T, F)
    assert sizes
    for T in sizes:
        a = mb.Atlas(T, F)
        rows = np.repeat(np.arange(F, dtype=np.float32), a.K)[:, None]
        tex = mb.host_atlas_scatter(a, rows, fill=-1000.0)
        assert int((tex[..., 0] == -1000.0).sum()) == T * T - F * a.K
        every = np.repeat(np.arange(F, dtype=np.int64), 6)
        fixed = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]]), (F, 1))
        face, bary = bc.queries(a, 2000, seed=T)
        face, bary = np.concatenate([every, face]), np.concatenate([fixed, bary])
        got = mb.host_atlas_sample(a, face, bary, tex)[:, 0]
        miss = (face < 0) | (face >= F)
        assert miss.any() and np.isnan(got[miss]).all()
        want = face[~miss].astype(np.float64)
        err = np.abs(got[~miss] - want)
        assert (err <= 4 * 2.0 ** -53 * want).all(), '%s, T = %d: %d of %d lookups leave their face, the worst by %g' % (
            name, T, int((err > 4 * 2.0 ** -53 * want).sum()), len(want), err.max())


@pytest.mark.parametrize('name', list(bc.meshes()))
def test_an_affine_field_is_reproduced(name):
    """f(p) = A p + b through host_atlas_points -> float32 rows -> scatter -> lookup at random barycentrics (b >= 0): within 2^-23 max|f|
    of f at the point -- which holds on the hypotenuse only because the gutter rows CONTINUE the plane instead of being clamped."""
    sizes, v, f, _ = fitting(name)
    for T in sizes:
        a = mb.Atlas(T, len(f))
        tex, top = bc.bake_affine(a, v, f)
        face, bary = bc.queries(a, 3000, seed=T + 1, misses=False)
        got = mb.host_atlas_sample(a, face, bary, tex)
        want = bc.affine(bc.surface_points(v, f, face, bary))
        err = np.abs(got - want).max()
        assert err <= 2.0 ** -23 * top, '%s, T = %d: %g > %g' % (name, T, err, 2.0 ** -23 * top)


def test_points_and_normals_of_the_rows():
    """Corner rows are the vertices themselves, rows inside are the barycentric points, gutter rows lie beyond the hypotenuse in the
    plane; normals are unit or exactly zero (a zero-area face, a zero vertex normal), never NaN; points_f32 is the rounded point."""
    for name, (v, f, vn) in bc.meshes().items():
        a = mb.Atlas(64, len(f))
        p, p32, nrm = mb.host_atlas_points(a, v, f, vn)
        assert p.shape == (len(f) * a.K, 3) and p.dtype == np.float64 and p32.dtype == np.float32 and np.array_equal(p32, p.astype(np.float32))
        i, j = a.local()
        P = p.reshape(len(f), a.K, 3)
        k_of = lambda ii, jj: jj * (a.n + 2) - jj * (jj - 1) // 2 + ii
        assert np.array_equal(P[:, k_of(0, 0)], v[f[:, 0]])
        for kk, corner in ((k_of(a.n, 0), 1), (k_of(0, a.n), 2)):
            assert np.abs(P[:, kk] - v[f[:, corner]]).max() <= 4 * 2.0 ** -53 * np.abs(v).max()
        b = np.stack([1.0 - (i + j) / a.n, i / a.n, j / a.n], axis=-1)                     # [K, 3], b0 = -1 / n on the gutter
        want = np.einsum('kc,fcd->fkd', b, v[f])
        assert np.abs(P - want).max() <= 16 * 2.0 ** -53 * np.abs(v).max() and (b[i + j == a.n + 1, 0] < 0).all()
        assert np.isfinite(nrm).all()
        length = np.linalg.norm(nrm, axis=1)
        assert (((np.abs(length - 1.0) <= 4 * 2.0 ** -53) | (length == 0.0))).all()
        if name == 'zero-area faces':
            assert not nrm.reshape(len(f), a.K, 3)[10:13].any() and (length.reshape(len(f), a.K)[:10] > 0).all()
        if name == 'a tetrahedron':
            assert (length == 0.0).any() and (length > 0).any()         # the row AT the vertex whose normal is zero
        if vn is None:
            geo = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
            ok = np.linalg.norm(geo, axis=1) > 1e-12
            unit = geo[ok] / np.linalg.norm(geo[ok], axis=1, keepdims=True)
            assert np.abs(nrm.reshape(len(f), a.K, 3)[ok] - unit[:, None, :]).max() <= 1e-14
        # a face range gives the same rows as the slice of the whole
        for f0, f1 in bc.face_ranges(len(f)):
            part = mb.host_atlas_points(a, v, f, vn, f0, f1)
            for whole, piece in zip((p, p32, nrm), part):
                assert np.array_equal(whole[f0 * a.K:f1 * a.K], piece)
    with pytest.raises(ValueError):
        mb.host_atlas_points(mb.Atlas(64, 1), np.zeros((3, 3)), np.array([[0, 1, 3]]))


def test_to_img_bytes():
    """The byte rule against (x.astype(float32).clip(0, 1) * 255).round().astype(uint8), on the .5 ties of x * 255, just beside them,
    below 0, above 1, at the infinities -- and NaN, whose byte is 0 BY THE RULE here (the expression leaves it to the conversion)."""
    x = bc.tie_values()
    assert np.isnan(x).any() and (x < 0).any() and (x > 1).any()
    prod = x[np.isfinite(x)] * np.float32(255.0)
    assert int((prod - np.floor(prod) == 0.5).sum()) >= 20                                # real ties, decided by half-to-even
    finite = ~np.isnan(x)
    with np.errstate(all='ignore'):
        want = (x.astype(np.float32).clip(0, 1) * 255).round().astype(np.uint8)
    got = mb.to_img(x)
    assert got.dtype == np.uint8 and np.array_equal(got[finite], want[finite]) and not got[~finite].any()
    a = mb.Atlas(64, 80)
    rows = bc.rows_for(80 * a.K, 3, seed=5)
    tex = mb.host_atlas_scatter(a, rows, fill=0.7, u8=True)
    xs, ys = a.texels()
    with np.errstate(all='ignore'):
        want = (np.where(np.isnan(rows), np.float32(0), rows).clip(0, 1) * 255).round().astype(np.uint8)
    assert tex.dtype == np.uint8 and np.array_equal(tex[ys, xs], want)
    free = a.owner()[0] < 0
    assert (tex[free] == int((np.float32(0.7) * 255).round())).all()
    from psnerf_amd import imgmetrics
    y = x[finite]
    assert np.array_equal(mb.to_img(y), imgmetrics.to_img(y))                             # the image code's rule, where that is defined


def test_chunks_compose_on_the_host():
    a = mb.Atlas(64, 79)
    rows = bc.rows_for(79 * a.K, 9, seed=2)
    whole = mb.host_atlas_scatter(a, rows, fill=0.25)
    tex = np.full((64, 64, 9), np.nan, dtype=np.float32)
    for n, (f0, f1) in enumerate(((0, 27), (27, 54), (54, 79))):
        mb.host_atlas_scatter(a, rows[f0 * a.K:f1 * a.K], f0, f1, out=tex, fill=0.25 if n == 0 else None)
    assert np.array_equal(tex.view(np.uint32), whole.view(np.uint32))


def parse_obj(path):
    v, vt, vn, faces, mtllib = [], [], [], [], None
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == 'v':
                v.append([float(t) for t in w[1:]])
            elif w[0] == 'vt':
                vt.append([float(t) for t in w[1:]])
            elif w[0] == 'vn':
                vn.append([float(t) for t in w[1:]])
            elif w[0] == 'f':
                faces.append([[int(t) if t else 0 for t in c.split('/')] for c in w[1:]])
            elif w[0] == 'mtllib':
                mtllib = w[1]
    return np.array(v), np.array(vt), np.array(vn), np.array(faces), mtllib


@pytest.mark.parametrize('name', ['icosphere(1)', 'icosphere(2)', 'an odd face count'])
def test_export_textured_round_trip(tmp_path, name):
    """The OBJ read back: 3 F vt, every index in range, the vt of face f are its three corner texels; the PNGs equal to_img of the maps
    (the normals as n / 2 + 0.5); the .mtl names files that exist; the specular weights come back from the .npy."""
    from PIL import Image
    v, f, vn = bc.meshes()[name]
    F, T = len(f), 64
    a = mb.Atlas(T, F)
    g = np.random.RandomState(1)
    baked = {'atlas': a, 'albedo': g.random_sample((T, T, 3)).astype(np.float32) * 1.2 - 0.1,
             'normal': (g.random_sample((T, T, 3)) * 2 - 1).astype(np.float32), 'specular': g.random_sample((T, T, 27)).astype(np.float32)}
    mesh = (v, f) if vn is None else (v, f, vn)
    files = mb.export_textured(str(tmp_path / 'out' / 'bear.obj'), mesh, baked)
    ov, ovt, ovn, of, mtllib = parse_obj(files['obj'])
    assert np.array_equal(ov, v) and ovt.shape == (3 * F, 2) and of.shape == (F, 3, 2 if vn is None else 3)
    assert np.array_equal(of[:, :, 0], f + 1) and np.array_equal(of[:, :, 1], np.arange(3 * F).reshape(F, 3) + 1)
    if vn is not None:
        assert len(ovn) == len(v) and np.array_equal(of[:, :, 2], f + 1) and np.abs(ovn - vn).max() < 1e-8
    x, y = ovt[:, 0] * T - 0.5, (1.0 - ovt[:, 1]) * T - 0.5                                  # back to texel centres
    texel = np.stack([np.rint(x), np.rint(y)], axis=-1).astype(np.int64).reshape(F, 3, 2)
    assert np.abs(x - np.rint(x)).max() < 1e-9 and np.abs(y - np.rint(y)).max() < 1e-9 and np.array_equal(texel, a.corners())
    owner = a.owner()[0]
    assert np.array_equal(owner[texel[..., 1], texel[..., 0]], np.repeat(np.arange(F)[:, None], 3, axis=1))
    assert mtllib == 'bear.mtl' and os.path.exists(files['mtl'])
    named = []
    with open(files['mtl']) as m:
        for line in m:
            w = line.split()
            if w and w[0] in ('map_Kd', 'norm', 'map_Bump'):
                named.append((w[0], w[-1]))
    assert ('map_Kd', 'bear_albedo.png') in named and any(k in ('norm', 'map_Bump') and n == 'bear_normal.png' for k, n in named)
    assert all(os.path.exists(os.path.join(os.path.dirname(files['mtl']), n)) for _, n in named)
    assert np.array_equal(np.asarray(Image.open(files['albedo'])), mb.to_img(baked['albedo']))
    assert np.array_equal(np.asarray(Image.open(files['normal'])), mb.to_img(baked['normal'] / np.float32(2) + np.float32(0.5)))
    assert np.array_equal(np.load(files['specular']), baked['specular'])
    g2 = mb.export_textured(str(tmp_path / 'gamma'), mesh, {'atlas': a, 'albedo': baked['albedo']}, gamma=2.2)
    want = mb.to_img(np.power(baked['albedo'].clip(0, 1), np.float32(1 / 2.2)).astype(np.float32))
    assert np.array_equal(np.asarray(Image.open(g2['albedo'])), want) and 'normal' not in g2 and g2['obj'].endswith('gamma.obj')


@pytest.mark.parametrize('case', list(bc.MODEL_CASES))
def test_bake_materials_on_the_host(case):
    """bake_materials of a CPU PSNetwork on icosphere(1) at 64 x 64 in chunks of 27 faces (27 + 27 + 26): every owned texel equals a
    direct, unchunked call of the same networks on the rows of host_atlas_points; unowned texels hold the fill; the albedo is within
    1e-4 of the oracle's network with the same state_dict at the same points."""
    from oracle import stage2 as o2
    net, onet = bc.make_models(case)
    net.train()
    v, f, vn = bc.meshes()['icosphere(1)']
    baked = mb.bake_materials(net, (v, f, vn), size=64, chunk_faces=27, fill=-2.0)
    assert net.training                                                   # (put back as it was)
    a = baked['atlas']
    assert (a.T, a.F) == (64, 80) and -(-a.F // 27) == 3 and a.F % 27 != 0
    sg = 'sgbasis' in case
    nets_normal = 'normal net' in case
    assert sorted(baked) == ['albedo', 'atlas', 'normal', 'specular']
    assert baked['albedo'].shape == (64, 64, 3) and baked['normal'].shape == (64, 64, 3) and baked['specular'].shape == (64, 64, 27 if sg else 1)
    assert all(baked[k].dtype == np.float32 for k in mb.MAPS)
    p, p32, nrm = mb.host_atlas_points(a, v, f, vn)
    x = torch.from_numpy(p32)
    with torch.no_grad():
        net.eval()
        direct = {'albedo': mb.eval_network(net, net.albedo_net, x, net.n_freqs), 'specular': mb.eval_network(net, net.rough_net, x, net.n_freqs)}
        if sg:
            direct['specular'] = torch.relu(direct['specular'])
        direct['normal'] = (torch.nn.functional.normalize(mb.eval_network(net, net.normal_net, x, net.n_freqs_n), dim=-1) if nets_normal
                            else torch.from_numpy(nrm).float())
        oracle_albedo = onet.albedo_net(o2.embed(x, 10)).numpy()
    xs, ys = a.texels()
    free = a.owner()[0] < 0
    for k in mb.MAPS:
        got, want = baked[k][ys, xs], direct[k].numpy()
        assert np.allclose(got, want, rtol=1e-5, atol=1e-5), '%s: %g' % (k, np.abs(got - want).max())
        assert (baked[k][free] == -2.0).all() and free.sum() == 64 * 64 - a.F * a.K
    if not nets_normal:
        assert np.array_equal(baked['normal'][ys, xs], nrm.astype(np.float32))
    err = np.abs(baked['albedo'][ys, xs] - oracle_albedo).max()
    assert err < 1e-4, err
    assert np.ptp(baked['albedo'][ys, xs]) > 1e-3                         # (not a constant: the points reach the network)
    only = mb.bake_materials(net, (v, f), size=64, maps=('albedo',), chunk_faces=80)
    assert sorted(only) == ['albedo', 'atlas'] and np.allclose(only['albedo'][ys, xs], direct['albedo'].numpy(), rtol=1e-5, atol=1e-5)
    assert not only['albedo'][free].any()
    with pytest.raises(ValueError):
        mb.bake_materials(net, (v, f), size=16)                           # 80 faces need 28 texels a side


def test_render_view_with_textures_on_the_host():
    """meshrender.render_view with textures= on the host path: the baked affine field comes back at the hit points, misses are NaN,
    and without textures the dict has exactly the keys it always had."""
    from psnerf_amd import meshrender as mr
    v, f, _ = bc.meshes()['icosphere(2)']
    a = mb.Atlas(256, len(f))
    tex, top = bc.bake_affine(a, v, f)
    H, W = 16, 20
    K, c2w = bc.view(H, W, fx=15.0)
    plain = mr.render_view((v, f), K, c2w, H, W)
    out = mr.render_view((v, f), K, c2w, H, W, textures={'field': tex}, atlas=a)
    assert sorted(plain) == ['depth', 'mask', 'normals', 'points', 't', 'tri'] and sorted(out) == sorted(list(plain) + ['field'])
    for k in plain:
        assert torch.equal(plain[k], out[k])
    mask = out['mask'].numpy()
    got = out['field'].numpy()
    assert got.shape == (H, W, 4) and 20 < mask.sum() < H * W and np.isnan(got[~mask]).all()
    want = bc.affine(out['points'].numpy()[mask])
    slack = 2.0 ** -23 * top + out['depth'].numpy()[mask] * 2.0 ** -52          # + the caster's own point error |t| 2^-52 |d|
    assert (np.abs(got[mask] - want).max(axis=-1) <= slack).all()
    with pytest.raises(ValueError):
        mr.render_view((v, f), K, c2w, H, W, textures={'field': tex})


def hocon(conf, indent=0):
    """A Conf tree as the text psnerf_amd.stage2.conf.parse_conf reads (sections, key = value, flat lists)."""
    pad, lines = '    ' * indent, []
    for key, val in conf.items():
        if isinstance(val, dict):
            lines += ['%s%s {' % (pad, key), hocon(val, indent + 1), '%s}' % pad]
        elif isinstance(val, (list, tuple)):
            lines.append('%s%s = [%s]' % (pad, key, ', '.join(str(x) for x in val)))
        else:
            lines.append('%s%s = %s' % (pad, key, str(val).lower() if isinstance(val, bool) else val))
    return '\n'.join(lines)


def test_bake_materials_tool_on_the_host(tmp_path):
    """tools/bake_materials.py --host: a mesh file, a conf file and a checkpoint directory as stage 2 writes it -> the textured OBJ,
    whose maps are those of bake_materials on the same model and mesh; tools/render_mesh.py --textures then looks them up."""
    import json
    import sys
    from PIL import Image
    import psnerf_amd.stage2 as s2
    from psnerf_amd.stage2.conf import parse_conf
    from psnerf_amd.stage1.extracting import Mesh
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import bake_materials as tool
    import render_mesh
    net, _ = bc.make_models('sgbasis, normal net')
    text = hocon(s2.bear_conf())
    assert parse_conf(text) == s2.bear_conf()
    (tmp_path / 'run.conf').write_text(text + '\n')
    os.makedirs(tmp_path / 'checkpoints' / 'ModelParameters')
    torch.save({'epoch': 7, 'model_state_dict': net.state_dict()}, str(tmp_path / 'checkpoints' / 'ModelParameters' / 'latest.pth'))
    v, f, _ = bc.meshes()['icosphere(2)']
    Mesh(v, f).export(str(tmp_path / 'mesh.obj'))
    files = tool.main(['--mesh', str(tmp_path / 'mesh.obj'), '--conf', str(tmp_path / 'run.conf'), '--checkpoint', str(tmp_path / 'checkpoints'),
                       '--out', str(tmp_path / 'baked' / 'ball.obj'), '--size', '128', '--host'])
    baked = mb.bake_materials(net, (v, f), size=128)
    assert np.array_equal(np.asarray(Image.open(files['albedo'])), mb.to_img(baked['albedo']))
    assert np.array_equal(np.asarray(Image.open(files['normal'])), mb.to_img(baked['normal'] / np.float32(2) + np.float32(0.5)))
    assert np.array_equal(np.load(files['specular']), baked['specular'])
    H, W = 24, 32
    K, c2w = bc.view(H, W, fx=20.0)
    pose = c2w[0].numpy().copy()
    pose[:3, 1:3] *= -1.0                                                  # the file holds OpenGL poses
    with open(tmp_path / 'params.json', 'w') as fh:
        json.dump({'K': K[0].numpy().tolist(), 'pose_c2w': [pose.tolist()], 'imhw': [H, W], 'n_view': 1}, fh)
    render_mesh.main(['--mesh', files['obj'], '--cameras', str(tmp_path / 'params.json'), '--out', str(tmp_path / 'maps'), '--textures', '--host'])
    mask = np.load(tmp_path / 'maps' / 'mask' / 'view_01.npy')
    albedo = np.load(tmp_path / 'maps' / 'tex_albedo' / 'view_01.npy')
    spec = np.load(tmp_path / 'maps' / 'tex_specular' / 'view_01.npy')
    assert 20 < mask.sum() < H * W and albedo.shape == (H, W, 3) and spec.shape == (H, W, 27)
    assert np.isnan(albedo[~mask]).all() and np.isfinite(albedo[mask]).all() and np.isfinite(spec[mask]).all()
    own = baked['albedo'][baked['atlas'].owner()[0] >= 0]
    assert albedo[mask].min() >= own.min() - 1.0 / 255 and albedo[mask].max() <= own.max() + 1.0 / 255     # bytes of the owned texels, blended
