"""The occlusion definition on the host (psnerf_amd/meshocclude.py: hemisphere_table, frame, host_occlusion_rows, occlusion_rows,
vertex_occlusion) and what is built on it (meshbake.bake_occlusion, bake_materials(occlusion=K), export_textured, the tools), checked
against facts that do not depend on the implementation: a convex mesh occludes nothing outside and everything inside, a corner occludes
half the cosine-weighted hemisphere, bits agree with single rays through meshdist.host_ray_cast."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import bake_cases as bc, occlusion_cases as oc, raycast_cases as rc
from psnerf_amd import meshbake as mb
from psnerf_amd import meshdist as md
from psnerf_amd import meshocclude as mo


# ------------------------------------------------------------------------------------------------ table and frame
@pytest.mark.parametrize('K', [1, 16, 64, 1024])
def test_hemisphere_table(K):
    t = mo.hemisphere_table(K)
    assert t.shape == (K, 3) and t.dtype == np.float64
    assert np.abs(np.linalg.norm(t, axis=1) - 1.0).max() <= 4e-16 and (t[:, 2] > 0.0).all()
    assert len(np.unique(t, axis=0)) == K
    # the mean z of a cosine-weighted set is 2 / 3; the stratified u = (k + 0.5) / K brings the mean of sqrt(1 - u) there like 1 / K
    assert abs(t[:, 2].mean() - 2.0 / 3.0) <= 0.2 / K
    if K == 64:
        assert abs(t[:, 2].mean() - 0.6668) < 5e-5
    with pytest.raises(ValueError):
        mo.hemisphere_table(0)


def test_frame_is_orthonormal_and_right_handed():
    g = np.random.RandomState(0)
    n = oc.unit(g.standard_normal((1000, 3)))
    tiny = 2.0 ** -26
    special = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, -0.0 - 1.0], [tiny, 0.0, -1.0 + 2.0 ** -52],
                        [0.0, -tiny, -1.0 + 2.0 ** -52], [1.0, 0.0, 0.0], [0.0, 1.0, -0.0], [-1.0, 0.0, 0.0]])
    n = np.concatenate([n, special])
    t, b = mo.frame(n)
    dot = lambda a, c: np.abs((a * c).sum(axis=1)).max()
    det = np.linalg.det(np.stack([t, b, n], axis=1))
    print('t.n %.2e  b.n %.2e  t.b %.2e  |t|-1 %.2e  |b|-1 %.2e  det-1 %.2e' % (
        dot(t, n), dot(b, n), dot(t, b), np.abs(np.linalg.norm(t, axis=1) - 1).max(), np.abs(np.linalg.norm(b, axis=1) - 1).max(), np.abs(det - 1).max()))
    assert np.isfinite(t).all() and np.isfinite(b).all()
    assert max(dot(t, n), dot(b, n), dot(t, b)) <= 5e-16
    assert np.abs(np.linalg.norm(t, axis=1) - 1.0).max() <= 5e-16 and np.abs(np.linalg.norm(b, axis=1) - 1.0).max() <= 5e-16
    assert np.abs(det - 1.0).max() <= 1e-15
    # the stated operation order, on one normal by hand
    nx, ny, nz = n[0]
    s = 1.0 if nz >= 0.0 else -1.0
    a = -1.0 / (s + nz)
    q = (nx * ny) * a
    assert np.array_equal(t[0], [1.0 + (s * (nx * nx)) * a, s * q, (-s) * nx]) and np.array_equal(b[0], [q, s + (ny * ny) * a, -ny])
    assert np.array_equal(mo.frame([0.0, 0.0, 1.0])[0], [1.0, 0.0, 0.0]) and np.array_equal(mo.frame([0.0, 0.0, -1.0])[1], [0.0, -1.0, 0.0])


# ------------------------------------------------------------------------------------------------ a convex mesh
def test_convex_mesh_outside_and_inside():
    """icosphere(2), three points per face, geometric normals, the default bias: nothing is blocked outside, everything inside, and
    with rays of 0.05 next to nothing (only a ray that grazes along the inside of the surface finds a face that close)."""
    v, f = rc.icosphere(2)
    K = 64
    p, n, face = oc.surface_rows(v, f, 3 * len(f), seed=1, face=np.repeat(np.arange(len(f)), 3))
    assert (np.bincount(face) == 3).all() and ((p * n).sum(axis=1) > 0).all()
    hits, visible, ao, bent, words = mo.occlusion_rows((v, f), p, n, K=K)
    assert hits.dtype == np.int32 and visible.dtype == np.int32 and ao.dtype == np.float64 and bent.shape == (len(p), 3) and words is None
    assert (hits == 0).all() and (visible == K).all() and (ao == 1.0).all()
    t = mo.hemisphere_table(K)
    # nothing blocked: the bent normal is the normalised sum of the whole table about n, which is n up to the table's own imbalance
    lean = np.linalg.norm(t[:, :2].sum(axis=0)) / t[:, 2].sum()
    assert np.abs(np.linalg.norm(bent, axis=1) - 1.0).max() <= 1e-15 and (1.0 - (bent * n).sum(axis=1)).max() <= lean ** 2
    inside = mo.occlusion_rows((v, f), p, -n, K=K)
    assert (inside[0] == K).all() and (inside[1] == 0).all() and (inside[2] == 0.0).all() and (inside[3] == 0.0).all()
    short = mo.occlusion_rows((v, f), p, -n, K=K, t_max=0.05)
    print('inside, t_max 0.05: at most %d of %d blocked' % (short[0].max(), K))
    assert (short[0] <= 3).all() and (short[0] + short[1] == K).all()


def test_vertex_occlusion_and_one_code_path():
    v, f = rc.icosphere(2)
    hits, visible, ao, bent, _ = mo.vertex_occlusion((v, f), K=16)
    assert hits.shape == (len(v),) and (hits == 0).all() and (visible == 16).all()
    vn = mo.area_weighted_normals(v, f)
    assert (1.0 - (vn * v).sum(axis=1)).max() < 1e-3                          # on a sphere the vertex is its normal
    inward = mo.vertex_occlusion((v, f), vertex_normals=-vn, K=16)
    assert (inward[0] == 16).all()
    # the mesh's own normals are used when it carries some
    assert (mo.vertex_occlusion((v, f, -vn), K=16)[0] == 16).all()
    # a ready host index, and the definition directly, give the same answer
    index = md._HostMesh(v, f)
    a = mo.occlusion_rows(index, v, vn, K=16, bits=True)
    b = mo.host_occlusion_rows(v, f, v, vn, mo.hemisphere_table(16), bias=mo.default_bias(index), bits=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert abs(mo.default_bias(index) / (1e-4 * np.linalg.norm(v.max(0) - v.min(0))) - 1.0) < 1e-15
    with pytest.raises(RuntimeError, match='CPU tensor'):
        mo.occlusion_rows((torch.from_numpy(v), torch.from_numpy(f)), v, vn)
    for bad in (dict(bias=np.nan), dict(t_max=-1.0), dict(t_max=np.nan), dict(table=np.zeros((0, 3))), dict(table=np.zeros((4, 2)))):
        with pytest.raises(ValueError):
            mo.occlusion_rows((v, f), v, vn, **bad)


# ------------------------------------------------------------------------------------------------ a corner
def test_corner_occludes_half():
    """At the foot of a wall the wall takes half of the cosine-weighted hemisphere: the directions with x < 0.  Farther from the wall
    it takes less and less."""
    v, f = oc.corner_mesh()
    up = np.array([[0.0, 0.0, 1.0]])
    for K in (16, 64, 256):
        share = [mo.occlusion_rows((v, f), np.array([[x, 0.1, 0.0]]), up, K=K, bias=1e-6)[0][0] / float(K) for x in (1e-3, 0.5, 1.0, 2.0, 5.0)]
        print('K = %3d: blocked share at x = 1e-3, 0.5, 1, 2, 5: %s' % (K, ', '.join('%.4f' % s for s in share)))
        assert abs(share[0] - 0.5) <= 2.0 / K
        assert all(a >= b for a, b in zip(share, share[1:]))
    hits, visible, ao, bent, _ = mo.occlusion_rows((v, f), np.array([[1e-3, 0.1, 0.0]]), up, K=256, bias=1e-6)
    assert bent[0, 0] > 0.2 and bent[0, 2] > 0.5 and ao[0] == 1.0 - hits[0] / 256.0          # the bent normal leans away from the wall


# ------------------------------------------------------------------------------------------------ world mode, bits
@pytest.mark.parametrize('K', [1, 31, 32, 33, 65])
def test_world_mode_and_bits(K):
    v, f = rc.icosphere(2)
    p, n, _ = oc.surface_rows(v, f, 40, seed=K)
    n[::2] = -n[::2]                                                            # half of the rows look inward
    table = oc.world_table(K, seed=K)
    bias = 1e-3
    hits, visible, ao, bent, words = mo.host_occlusion_rows(v, f, p, n, table, local=False, bias=bias, t_max=1.2, bits=True)
    assert words.shape == (40, (K + 31) // 32) and words.dtype == np.int32
    facing = (n[:, None, 0] * table[None, :, 0] + n[:, None, 1] * table[None, :, 1]) + n[:, None, 2] * table[None, :, 2] > 0.0
    assert np.array_equal(hits + visible, facing.sum(axis=1))
    seen = mo.unpack_bits(words, K)
    assert seen.shape == (40, K) and not seen[~facing].any()                   # what does not face the normal is never cast: bit 0
    blocked = np.stack([md.host_ray_cast(v, f, p + bias * n, np.broadcast_to(table[k], p.shape), 0.0, 1.2, any_hit=True)[3] for k in range(K)], axis=1)
    assert np.array_equal(seen, facing & ~blocked) and np.array_equal(hits, (facing & blocked).sum(axis=1))
    assert np.array_equal(visible, seen.sum(axis=1))
    pad = np.arange(words.shape[1] * 32).reshape(1, -1, 32) >= K                 # the bits beyond K stay 0
    raw = (words.view(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    assert not raw[np.broadcast_to(pad, raw.shape)].any()
    with np.errstate(invalid='ignore', divide='ignore'):
        assert np.array_equal(ao, np.where(facing.sum(1) > 0, 1.0 - hits / np.maximum(facing.sum(1), 1), 1.0))
    # the bent normal: the sequential sum of the unblocked cast directions, normalised
    for r in range(0, 40, 7):
        m = np.zeros(3)
        for k in range(K):
            if seen[r, k]:
                m = m + table[k]
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        assert np.array_equal(bent[r], m / length if length > 0 else np.zeros(3))
    # bits off: the same numbers, no words
    again = mo.host_occlusion_rows(v, f, p, n, table, local=False, bias=bias, t_max=1.2)
    assert again[4] is None and all(np.array_equal(x, y) for x, y in zip(again[:4], (hits, visible, ao, bent)))


def test_degenerate_rows():
    v, f = rc.icosphere(2)
    p, n, _ = oc.surface_rows(v, f, 24, seed=3)
    p, n, dead = oc.degenerate_rows(p, n)
    assert dead.sum() == 5
    for local, table in ((True, mo.hemisphere_table(33)), (False, oc.world_table(33, 1))):
        hits, visible, ao, bent, words = mo.host_occlusion_rows(v, f, p, n, table, local=local, bias=1e-3, bits=True)
        assert (hits[dead] == -1).all() and np.isnan(ao[dead]).all() and (bent[dead] == 0.0).all() and (visible[dead] == 0).all()
        assert (words[dead] == 0).all()
        assert (hits[~dead] >= 0).all() and np.isfinite(ao[~dead]).all()
    # K' = 0: no direction of the table faces the normal -> nothing cast, ao = 1, bent = 0
    up = np.tile([0.0, 0.0, 1.0], (3, 1))
    away = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.6, 0.0, -0.8], [0.0, -1.0, -0.0]])      # below the horizon, or exactly in it
    hits, visible, ao, bent, words = mo.host_occlusion_rows(v, f, p[:3], up, away, local=False, bits=True)
    assert (hits == 0).all() and (visible == 0).all() and (ao == 1.0).all() and (bent == 0.0).all() and (words == 0).all()


# ------------------------------------------------------------------------------------------------ bake and export
def test_bake_occlusion_on_the_host_chunks_compose():
    """icosphere(1) with vertex normals at 64 x 64, K = 8: one call == chunks of 27 faces == chunks of 1 face, bit for bit; the texels are
    the rows of occlusion_rows at atlas_points' points and normals; a zero normal bakes ``fill``."""
    v, f, vn = bc.meshes()['icosphere(1)']
    T, K = 64, 8
    one = mb.bake_occlusion((v, f, vn), size=T, K=K, fill=0.25)
    a = one['atlas']
    assert set(one) == {'atlas', 'occlusion', 'bent'} and one['occlusion'].shape == (T, T, 1) and one['bent'].shape == (T, T, 3)
    assert one['occlusion'].dtype == np.float32 and one['bent'].dtype == np.float32
    for chunk in (27, 1):
        parts = mb.bake_occlusion((v, f, vn), atlas=a, K=K, fill=0.25, chunk_faces=chunk)
        assert np.array_equal(parts['occlusion'], one['occlusion']) and np.array_equal(parts['bent'], one['bent'])
    p, _, n = mb.host_atlas_points(a, v, f, vn)
    hits, _, ao, bent, _ = mo.occlusion_rows((v, f), p, n, K=K)
    x, y = a.texels()
    assert np.array_equal(one['occlusion'][y, x, 0], ao.astype(np.float32)) and np.array_equal(one['bent'][y, x], bent.astype(np.float32))
    free = a.owner()[0] < 0
    assert (one['occlusion'][free] == 0.25).all() and (one['bent'][free] == 0.25).all() and free.any()
    assert 0.0 < one['occlusion'][~free].min() and one['occlusion'][~free].max() == 1.0
    tv, tf, tn = bc.meshes()['a tetrahedron']                                  # vertex 3 has a zero normal: the rows AT it cast nothing
    tet = mb.bake_occlusion((tv, tf, tn), size=16, K=8, fill=0.5)
    rows_n = mb.host_atlas_points(tet['atlas'], tv, tf, tn)[2]
    dead = ~(rows_n != 0.0).any(axis=1)
    tx, ty = tet['atlas'].texels()
    assert dead.any() and (tet['occlusion'][ty[dead], tx[dead], 0] == 0.5).all() and (tet['bent'][ty[dead], tx[dead]] == 0.5).all()
    with pytest.raises(ValueError):
        mb.bake_occlusion((v, f, vn), atlas=mb.Atlas(64, 79), K=K)


def _read(files):
    return dict((k, open(p, 'rb').read()) for k, p in files.items())


def test_export_textured_with_and_without_occlusion(tmp_path):
    """Without the new keys export_textured writes what it always wrote; with them the same bytes, plus name_ao.png, name_bent.png and
    their lines at the end of the MTL."""
    from PIL import Image
    v, f, vn = bc.meshes()['icosphere(1)']
    T = 64
    a = mb.Atlas(T, len(f))
    g = np.random.RandomState(2)
    plain = {'atlas': a, 'albedo': g.random_sample((T, T, 3)).astype(np.float32), 'normal': (g.random_sample((T, T, 3)) * 2 - 1).astype(np.float32),
             'specular': g.random_sample((T, T, 27)).astype(np.float32)}
    occ = mb.bake_occlusion((v, f, vn), atlas=a, K=8)
    both = dict(plain, occlusion=occ['occlusion'], bent=occ['bent'])
    without = mb.export_textured(str(tmp_path / 'a' / 'bear.obj'), (v, f, vn), plain)
    with_keys = mb.export_textured(str(tmp_path / 'b' / 'bear.obj'), (v, f, vn), both)
    assert set(without) == {'obj', 'mtl', 'albedo', 'normal', 'specular'} and set(with_keys) == set(without) | {'ao', 'bent'}
    assert sorted(os.listdir(tmp_path / 'a')) == ['bear.mtl', 'bear.obj', 'bear_albedo.png', 'bear_normal.png', 'bear_specular.npy']
    old, new = _read(without), _read(with_keys)
    for key in ('obj', 'albedo', 'normal', 'specular'):
        assert old[key] == new[key], key
    assert old['mtl'] == (b'newmtl bear\nKa 0 0 0\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd bear_albedo.png\n# object-space normals, stored as n / 2 + 0.5\n'
                          b'norm bear_normal.png\n# specular: bear_specular.npy, float32 [T, T, C]\n')
    assert new['mtl'].startswith(old['mtl'])
    added = new['mtl'][len(old['mtl']):].decode().splitlines()
    assert 'map_Ka bear_ao.png' in added and any(line.startswith('#') and 'bear_bent.png' in line for line in added)
    assert sum(not line.startswith('#') for line in added) == 1 and any(line.startswith('#') and 'occlusion' in line for line in added)
    ao_png, bent_png = np.asarray(Image.open(with_keys['ao'])), np.asarray(Image.open(with_keys['bent']))
    assert ao_png.shape == (T, T) and np.array_equal(ao_png, mb.to_img(occ['occlusion'])[:, :, 0])
    assert np.array_equal(bent_png, mb.to_img(occ['bent'] / np.float32(2) + np.float32(0.5)))
    only = mb.export_textured(str(tmp_path / 'c' / 'bear'), (v, f, vn), {'atlas': a, 'occlusion': occ['occlusion']})
    assert set(only) == {'obj', 'mtl', 'ao'}


def test_bake_materials_with_occlusion_and_the_tools(tmp_path):
    """bake_materials(..., occlusion=K) on the host: the material maps are untouched and the two new maps are bake_occlusion's on the same
    atlas; tools/bake_materials.py --occlusion writes them and tools/render_mesh.py --textures looks them up."""
    import json
    from PIL import Image
    import psnerf_amd.stage2 as s2
    from psnerf_amd.stage1.extracting import Mesh
    from tests.test_bake_cpu import hocon
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import bake_materials as tool
    import render_mesh
    net, _ = bc.make_models('sgbasis, geometric normals')
    v, f, _ = bc.meshes()['icosphere(1)']
    T, K = 64, 8
    plain = mb.bake_materials(net, (v, f), size=T, maps=('albedo',))
    both = mb.bake_materials(net, (v, f), size=T, maps=('albedo',), occlusion=K, occlusion_distance=1.5, chunk_faces=27)
    occ = mb.bake_occlusion((v, f), size=T, K=K, t_max=1.5)
    assert set(plain) == {'atlas', 'albedo'} and set(both) == {'atlas', 'albedo', 'occlusion', 'bent'}
    assert np.array_equal(plain['albedo'], both['albedo'])
    assert np.array_equal(both['occlusion'], occ['occlusion']) and np.array_equal(both['bent'], occ['bent'])
    (tmp_path / 'run.conf').write_text(hocon(s2.bear_conf(**bc.MODEL_CASES['sgbasis, geometric normals'])) + '\n')
    os.makedirs(tmp_path / 'checkpoints' / 'ModelParameters')
    torch.save({'epoch': 7, 'model_state_dict': net.state_dict()}, str(tmp_path / 'checkpoints' / 'ModelParameters' / 'latest.pth'))
    Mesh(v, f).export(str(tmp_path / 'mesh.obj'))
    files = tool.main(['--mesh', str(tmp_path / 'mesh.obj'), '--conf', str(tmp_path / 'run.conf'), '--checkpoint', str(tmp_path / 'checkpoints'),
                       '--out', str(tmp_path / 'baked' / 'ball.obj'), '--size', str(T), '--maps', 'albedo', '--host', '--occlusion', str(K),
                       '--occlusion-distance', '1.5'])
    assert np.array_equal(np.asarray(Image.open(files['ao'])), mb.to_img(occ['occlusion'])[:, :, 0])
    assert np.array_equal(np.asarray(Image.open(files['bent'])), mb.to_img(occ['bent'] / np.float32(2) + np.float32(0.5)))
    H, W = 24, 32
    cam, c2w = bc.view(H, W, fx=20.0)
    pose = c2w[0].numpy().copy()
    pose[:3, 1:3] *= -1.0                                                  # the file holds OpenGL poses
    with open(tmp_path / 'params.json', 'w') as fh:
        json.dump({'K': cam[0].numpy().tolist(), 'pose_c2w': [pose.tolist()], 'imhw': [H, W], 'n_view': 1}, fh)
    render_mesh.main(['--mesh', files['obj'], '--cameras', str(tmp_path / 'params.json'), '--out', str(tmp_path / 'maps'), '--textures', '--host'])
    mask = np.load(tmp_path / 'maps' / 'mask' / 'view_01.npy')
    shown = np.load(tmp_path / 'maps' / 'tex_occlusion' / 'view_01.npy')
    bent = np.load(tmp_path / 'maps' / 'tex_bent' / 'view_01.npy')
    assert 20 < mask.sum() < H * W and shown.shape == (H, W, 1) and bent.shape == (H, W, 3)
    assert np.isnan(shown[~mask]).all() and (shown[mask] == 1.0).all()          # a convex mesh: open everywhere, byte 255 in every owned texel
    assert os.path.exists(tmp_path / 'maps' / 'tex_occlusion' / 'view_01.png')
